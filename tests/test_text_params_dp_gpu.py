"""Data-parallel gradient exchange with `args.text_params = "flat"`: two processes share cuda:0 and talk over gloo, as in
test_dp_gpu.py.  Each rank runs the SAME model (tiny BERT on the HIP path in front of the toy trunk) on its half of a batch,
as TWO accumulation micro-steps of which only the second exchanges, with distributed.GradSync hooked in: the text backward
reports its sections (layer 1, layer 0, embeddings) as it finishes them and they are all-reduced in place on the
communication stream.  Afterwards every parameter's gradient must equal the gradient of the mean loss over the global
batch, computed by the same process in one pass without any exchange.

Measure: max |got - ref| / max(max |ref|, floor) per tensor, floor = 1e-3 of the model's largest gradient (the measure of
test_text_encoder_gpu.py: a key bias's exact gradient is zero).  Bound 2e-4, test_dp_gpu.py's for the f32 exchange: the
shards and micro-steps only change the order of fp32 sums."""
import os
import socket
import sys

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
pytestmark = pytest.mark.gpu


def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


def _worker(rank, world, port, bert_dir, out):
    sys.path.insert(0, ROOT)
    sys.path.insert(0, os.path.join(ROOT, "tests"))
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    os.environ.setdefault("HSA_ENABLE_IPC_MODE_LEGACY", "0")
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bpmult_amd  # noqa: F401
    from types import SimpleNamespace
    from bpmult_amd.distributed import GradSync
    from bpmult_amd.models import get_model
    from test_text_encoder_gpu import model_args
    torch.manual_seed(5)
    model = get_model(model_args(bert_dir, orig_d_l=32, text_encoder="hip", text_embeddings="hip", text_params="flat"))
    model = model.cuda().train()
    g = torch.Generator().manual_seed(9)
    B, L = 8, 12
    ids = torch.randint(1, 60, (B, L), generator=g)
    mask = torch.ones(B, L, dtype=torch.long)
    mask[1, 7:] = 0
    mask[6, 3:] = 0
    ids = (ids * mask).cuda()
    mask, seg = mask.cuda(), torch.zeros(B, L, dtype=torch.long).cuda()
    img, aud = torch.randn(B, 40, 35, generator=g).cuda(), torch.randn(B, 31, 74, generator=g).cuda()
    tgt = (torch.randn(B, 6, generator=g) > 0).float().cuda()
    opt = SimpleNamespace(pending_grad_scale=None)
    sync = GradSync(model, bucket_bytes=1 << 14, optimizer=opt)        # small buckets: several all-reduces per section

    def backward(sl, scale=1.0):
        logits = model(ids[sl], mask[sl], seg[sl], img[sl], aud[sl])
        (torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt[sl]) * scale).backward()

    sync.active = False
    backward(slice(0, B))
    torch.cuda.synchronize()
    full = {k: p.grad.detach().clone() for k, p in model.named_parameters() if p.grad is not None}
    text = model.enc.flat_store()
    assert len(model._flat_stores()) == 2 and any(k in text.params for k in full)
    for p in model.parameters():
        p.grad = None
    seen = []
    real = sync._exchange
    sync._exchange = lambda flat, lo, hi: (seen.append((flat.data_ptr() == text.gflat.data_ptr(), lo, hi)), real(flat, lo, hi))[1]
    per = B // world
    half = per // 2
    for j, active in ((0, False), (1, True)):
        sync.active = active
        lo = rank * per + j * half
        backward(slice(lo, lo + half), 0.5)
        assert bool(seen) == active
        sync.finish()
    torch.cuda.synchronize()
    assert [s[1:] for s in seen if s[0]] == [text.sections[k] for k in ("layer1", "layer0", "embeddings")]
    assert opt.pending_grad_scale == 1.0 / world                           # the buffers keep the SUM
    floor = 1e-3 * max(float(t.abs().max()) for t in full.values())
    worst, where = 0.0, None
    for k, p in model.named_parameters():
        if k in full:
            e = float((p.grad / world - full[k]).abs().max() / max(float(full[k].abs().max()), floor))
            if e > worst:
                worst, where = e, k
    out[rank] = (worst, where)
    dist.destroy_process_group()


def test_gradsync_two_ranks_with_a_flat_text_store(tmp_path):
    from test_text_params_gpu import tiny_bert
    d = str(tmp_path / "bert")
    tiny_bert().save_pretrained(d)
    world = 2
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, d, out), nprocs=world, join=True)
    assert len(out) == world
    for r, (e, where) in out.items():
        print("rank", r, "worst gradient", e, where)
        assert e < 2e-4, (r, e, where)
