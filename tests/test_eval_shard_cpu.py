"""Sharded evaluation, the parts that need no GPU: how the batches are dealt to the ranks, the argument checks, the no-op
of Evaluator.all_gather outside a group, and fit(process_group=...) between two gloo ranks on the CPU -- one writer, every
rank behind the write, the same history and the same restored state everywhere."""
import datetime
import os
import socket
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bpmult_amd  # noqa: F401
from bpmult_amd import metrics, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
LIMIT = datetime.timedelta(seconds=60)


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def test_shard_range_deals_contiguous_shares_once():
    for n in range(0, 21):
        for world in range(1, 10):
            spans = [training.shard_range(n, world, r) for r in range(world)]
            assert spans[0][0] == 0 and spans[-1][1] == n
            assert all(a[1] == b[0] for a, b in zip(spans, spans[1:]))          # ordered, no gap, no overlap
            sizes = [hi - lo for lo, hi in spans]
            assert min(sizes) >= 0 and max(sizes) - min(sizes) <= 1 and sum(sizes) == n
    assert [training.shard_range(2, 3, r) for r in range(3)] == [(0, 0), (0, 1), (1, 2)]       # n < world: empty shares
    for bad in ((-1, 2, 0), (4, 0, 0), (4, 2, 2), (4, 2, -1)):
        with pytest.raises(ValueError, match="shard_range"):
            training.shard_range(*bad)


def test_argument_checks_of_model_eval_and_make_evaluate():
    args = SimpleNamespace(task="mmimdb", task_type="multilabel", model="mmtrvat", n_classes=6)
    assert not dist.is_initialized()
    with pytest.raises(ValueError, match="presharded"):
        training.model_eval(None, None, [], args, presharded=True)
    with pytest.raises(ValueError, match="not initialised"):
        training.model_eval(None, None, [], args, process_group=object())
    with pytest.raises(ValueError, match="not initialised"):
        training.make_evaluate(None, lambda: [], args, "auc_pr_micro", process_group=object())
    with pytest.raises(ValueError, match="not initialised"):
        training.fit(None, None, None, lambda: [], None, None, "unused", 1, 1, process_group=object())
    ev = training.make_evaluate(None, lambda: [], args, "auc_pr_micro")            # today's call still builds
    assert callable(ev) and ev.metrics is None


def test_all_gather_is_a_no_op_without_a_group_and_in_a_world_of_one():
    ev = metrics.Evaluator.__new__(metrics.Evaluator)      # no store (that needs a GPU): a no-op touches none of it
    assert not dist.is_initialized()
    assert ev.all_gather() is None and ev.all_gather(counts=[(3, 1)]) is None
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{_free_port()}", rank=0, world_size=1, timeout=LIMIT)
    try:
        assert ev.all_gather() is None and ev.all_gather(dist.group.WORLD, [(3, 1)]) is None
        assert vars(ev) == {}
    finally:
        dist.destroy_process_group()


METRICS = [0.1, 0.3, 0.2, 0.25, 0.9]          # improves twice, stalls twice: stops after epoch 3 at patience 2


def _fit_worker(rank, world, port, out, savedir):
    sys.path.insert(0, ROOT)
    dist.init_process_group("gloo", init_method=f"tcp://127.0.0.1:{port}", rank=rank, world_size=world, timeout=LIMIT)
    import bpmult_amd  # noqa: F401
    from bpmult_amd import training as tr
    group = dist.group.WORLD
    written = []
    save = tr.save_checkpoint
    tr.save_checkpoint = lambda state, is_best, path, *a: (written.append(state["epoch"]), save(state, is_best, path, *a))

    ck_path = os.path.join(savedir, "checkpoint.pt")
    real_exists = os.path.exists

    def run(max_epochs, seed, rank1_sees):
        # rank 1's own look at the save directory is made WRONG on purpose (a rank that arrives after rank 0's first write
        # sees a file at a fresh start; a lagging shared file system hides one at a resume): the decision is rank 0's
        if rank == 1:
            os.path.exists = lambda p: rank1_sees if p == ck_path else real_exists(p)
        try:
            return run_fit(max_epochs, seed)
        finally:
            os.path.exists = real_exists

    def run_fit(max_epochs, seed):
        torch.manual_seed(seed)
        model = torch.nn.Linear(4, 2)
        opt = torch.optim.SGD(model.parameters(), lr=0.1)
        sched = tr.get_scheduler(opt, 0, 0.5)
        it = iter(METRICS)
        xs = [torch.ones(3, 4) * (i + 1) for i in range(2)]
        r = tr.fit(model, opt, sched, lambda: xs, lambda m, b: m(b).pow(2).mean(), lambda m: next(it), savedir, max_epochs, 2,
                   process_group=group)
        return model, r

    _, first = run(10, 1, True)
    files = sorted(os.listdir(savedir))
    ck = torch.load(os.path.join(savedir, "checkpoint.pt"), map_location="cpu", weights_only=False)
    # resumed at the checkpoint's epoch with other initial weights on every rank: nothing left to run, the state restored
    model, again = run(ck["epoch"], 100 + rank, False)
    restored = all(torch.equal(v, ck["state_dict"][k]) for k, v in model.state_dict().items())
    out[rank] = {"history": first["history"], "best": first["best_metric"], "written": written, "files": files,
                 "ck_epoch": ck["epoch"], "restored": restored, "again": (again["epochs_run"], again["best_metric"])}
    dist.destroy_process_group()


def test_fit_two_ranks_one_writer_same_history_and_resume(tmp_path):
    world = 2
    out = mp.Manager().dict()
    mp.spawn(_fit_worker, args=(world, _free_port(), out, str(tmp_path)), nprocs=world, join=True)
    r0, r1 = out[0], out[1]
    assert r0["history"] == r1["history"] and r0["best"] == r1["best"] == 0.3
    assert [h["improved"] for h in r0["history"]] == [True, True, False, False]            # stopped by patience, in step
    assert [h["lr"] for h in r0["history"]] == [0.1, 0.1, 0.05, 0.025]
    assert r0["written"] == [1, 2] and r1["written"] == []                                 # only rank 0 writes
    assert r0["files"] == r1["files"] == ["checkpoint.pt", "model_best.pt"]
    for r in (r0, r1):
        assert r["ck_epoch"] == 2 and r["restored"] and r["again"] == (0, 0.3)
