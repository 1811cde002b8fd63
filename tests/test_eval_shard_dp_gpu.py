"""Sharded evaluation across ranks: two processes share cuda:0 and talk over gloo (the pattern of tests/test_dp_gpu.py;
with two GPUs the same worker runs once more over RCCL, one GPU per rank).

Each rank builds the same tiny mmtrvat (f32, eval mode) and the same five batches of sizes [3, 2, 3, 1, 2], and runs
training.model_eval with and without the process group.  Both computations push the same batches through the same
deterministic eval-mode kernels on the same device and only bit patterns are exchanged, so the dicts are compared with
==: no tolerance.  One spawn runs every scenario (the spawn and the model build are what cost time); the tests below look
at what the ranks reported."""
import datetime
import os
import socket
import sys

import numpy as np
import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu
SIZES = [3, 2, 3, 1, 2]


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _batches(sizes, Cn=6):
    g = torch.Generator().manual_seed(23)
    out = []
    for B in sizes:
        zeros = torch.zeros(B, 10, dtype=torch.long)
        out.append((torch.randn(B, 10, 32, generator=g), zeros, zeros, torch.randn(B, 20, 35, generator=g),
                    (torch.rand(B, Cn, generator=g) > 0.5).float(), torch.randn(B, 30, 74, generator=g)))
    return out


def _worker(rank, world, port, out, backend, savedir):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    limit = datetime.timedelta(seconds=60)          # a protocol mistake ends as an error, not as a hang
    if backend == "nccl":
        torch.cuda.set_device(rank)
        dist.init_process_group("nccl", rank=rank, world_size=world, timeout=limit, device_id=torch.device("cuda", rank))
    else:
        dist.init_process_group("gloo", rank=rank, world_size=world, timeout=limit)
    group = dist.group.WORLD
    import bpmult_amd  # noqa: F401
    from bpmult_amd import losses, metrics, training
    from bpmult_amd.distributed import GradSync
    from bpmult_amd.models import get_model
    from bpmult_amd.optim import FusedAdam
    from test_model_gpu import args_for
    torch.manual_seed(5)
    args = args_for("mmtrvat", hidden_sz=24, num_heads=4, layers=2, orig_d_l=32, num_vectors_l=32, num_vectors_a=32, num_vectors_v=32,
                    precision="f32", task="mmimdb", task_type="multilabel")
    model = get_model(args).cuda().eval()
    batches = _batches(SIZES)
    crit = losses.BCEWithLogitsLoss()
    calls = [0]

    def counting(o, t):
        calls[0] += 1
        return crit(o, t)

    res = {}
    # the whole list on every rank, sharded by model_eval
    res["plain"] = training.model_eval(model, crit, batches, args)
    res["sharded"] = training.model_eval(model, counting, batches, args, process_group=group)
    res["forwards"] = calls[0]
    # gates kept: gathered in rank order, dtype and bits unchanged
    ev0 = metrics.Evaluator("multilabel", 6, sum(SIZES), device="cuda")
    ev1 = metrics.Evaluator("multilabel", 6, sum(SIZES), device="cuda")
    a = training.model_eval(model, crit, batches, args, evaluator=ev0, output_gates=True)
    b = training.model_eval(model, crit, batches, args, evaluator=ev1, output_gates=True, process_group=group)
    p0, p1 = ev0.predictions(), ev1.predictions()
    res["gates"] = a == b and len(p1) == 4 and all(x.dtype == y.dtype and np.array_equal(x.view(np.uint8), y.view(np.uint8))
                                                     for x, y in zip(p0, p1))
    # a sharding loader: the batches passed are this rank's share
    lo, hi = training.shard_range(len(batches), world, rank)
    res["presharded"] = training.model_eval(model, crit, batches[lo:hi], args, process_group=group, presharded=True)
    # one batch in a world of two: rank 1 holds nothing
    res["single_plain"] = training.model_eval(model, crit, batches[:1], args)
    res["single"] = training.model_eval(model, crit, batches[:1], args, process_group=group)
    # ... and cannot know on its own that rank 0 keeps gates
    ev2 = metrics.Evaluator("multilabel", 6, 8, device="cuda")
    res["single_gates_plain"] = training.model_eval(model, crit, batches[:1], args, output_gates=True)
    res["single_gates"] = training.model_eval(model, crit, batches[:1], args, evaluator=ev2, output_gates=True, process_group=group)
    res["single_gates_rows"] = ev2.predictions()[3].shape[0]
    # C differs between the ranks: both raise, nobody waits
    Cn = 6 - rank
    ev = metrics.Evaluator("multilabel", Cn, 8, device="cuda")
    ev.update(torch.zeros(2, Cn, device="cuda"), torch.zeros(2, Cn, device="cuda"))
    try:
        ev.all_gather(group)
        res["mismatch"] = "no error"
    except ValueError as e:
        res["mismatch"] = str(e)
    # counts promised wrongly for rank 1 alone: it takes part in the collectives with a voided image and raises afterwards;
    # rank 0 does not wait, and learns of it at its one host read
    ev = metrics.Evaluator("multilabel", 6, 8, device="cuda")
    ev.update(torch.zeros(2, 6, device="cuda"), torch.zeros(2, 6, device="cuda"))
    try:
        ev.all_gather(group, [(2, 1, 0), (3, 1, 0)])
        ev.compute()
        res["broken"] = "no error"
    except ValueError as e:
        res["broken"] = str(e)
    # gates on rank 0 only, with counts given and the caller saying that gates are kept: both raise, nobody waits
    ev = metrics.Evaluator("multilabel", 6, 8, device="cuda")
    ev.update(torch.zeros(2, 6, device="cuda"), torch.zeros(2, 6, device="cuda"), None, torch.ones(2, 4, device="cuda") if rank == 0 else None)
    try:
        ev.all_gather(group, [(2, 1, 0), (2, 1, 0)], gates=True)
        res["mixture"] = "no error"
    except ValueError as e:
        res["mixture"] = str(e)
    # nothing stored anywhere: the collectives run, compute() refuses on every rank
    ev = metrics.Evaluator("multilabel", 6, 8, device="cuda")
    ev.all_gather(group)
    try:
        ev.compute()
        res["empty"] = "no error"
    except ValueError as e:
        res["empty"] = str(e)
    # fit() with GradSync, a sharded evaluate and the group: every validation batch is forwarded on exactly one rank
    calls[0] = 0
    opt = FusedAdam(model, lr=1e-3)
    sched = training.get_scheduler(opt, 2, 0.5)
    sync = GradSync(model, optimizer=opt)
    ev_fn = training.make_evaluate(counting, lambda: batches, args, "auc_pr_micro", process_group=group)
    train = [b for b, n in zip(batches, SIZES) if n == 2]
    r = training.fit(model, opt, sched, lambda: train, lambda m, b: training.model_forward(m, crit, b, "mmtrvat")[0], ev_fn, savedir,
                     max_epochs=2, patience=5, grad_sync=sync, process_group=group)
    res["fit_forwards"] = calls[0]
    res["fit_history"] = [(h["metric"], h["lr"], h["improved"]) for h in r["history"]]
    res["fit_metrics"] = ev_fn.metrics
    torch.cuda.synchronize()
    out[rank] = res
    dist.destroy_process_group()


def _run(backend, savedir):
    world = 2
    mgr = mp.Manager()
    out = mgr.dict()
    mp.spawn(_worker, args=(world, _free_port(), out, backend, savedir), nprocs=world, join=True)
    assert len(out) == world
    return [out[r] for r in range(world)]


def _check(ranks, savedir):
    r0, r1 = ranks
    for k in ("plain", "sharded", "presharded", "single", "single_plain", "single_gates", "fit_metrics", "fit_history"):
        assert r0[k] == r1[k], (k, r0[k], r1[k])
    for r in ranks:
        assert r["sharded"] == r["plain"] and r["presharded"] == r["plain"], (r["sharded"], r["presharded"], r["plain"])
        assert all(np.isfinite(v) for v in r["plain"].values()) and r["gates"] is True
        assert r["single"] == r["single_plain"] and r["single_gates"] == r["single_gates_plain"] and r["single_gates_rows"] == SIZES[0]
        assert "kind / C differ" in r["mismatch"] and "no rows" in r["empty"] and "kept on some ranks only" in r["mixture"]
    assert "voided its shard" in r0["broken"] and "rank 1 was promised" in r1["broken"]
    # five batches over two ranks: [0, 2) and [2, 5); two epochs of fit()
    assert (r0["forwards"], r1["forwards"]) == (2, 3)
    assert (r0["fit_forwards"], r1["fit_forwards"]) == (4, 6)
    assert len(r0["fit_history"]) == 2
    assert sorted(os.listdir(savedir)) == ["checkpoint.pt", "model_best.pt"]


@pytest.fixture(scope="module")
def gloo_ranks(tmp_path_factory):
    savedir = str(tmp_path_factory.mktemp("shard_gloo"))
    return _run("gloo", savedir), savedir


def test_two_ranks_return_the_unsharded_dict(gloo_ranks):
    _check(*gloo_ranks)


@pytest.mark.skipif(torch.cuda.device_count() < 2, reason="needs two GPUs (RCCL over xGMI); the one-GPU box runs the gloo variant above")
def test_sharded_evaluation_rccl_two_gpus(tmp_path):
    _check(_run("nccl", str(tmp_path)), str(tmp_path))
