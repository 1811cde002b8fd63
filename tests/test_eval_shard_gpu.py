"""Sharded evaluation on one GPU: bpm_eval_pack / bpm_eval_merge through metrics.Evaluator.pack / merge.

A batch list is split over W simulated shards, each with its own Evaluator; their images are merged into one destination,
which is compared with one Evaluator that was fed every batch in order.  Only bit patterns move, so there is no tolerance
here: every store array over the N rows (floats compared as their int32 bit patterns, so -0.0 is not 0.0 and a NaN is
itself), the losses, the counter of refused targets, compute() and predictions() are EQUAL.

Shapes: 256 elements per block of the merge kernel (an element is a row's class for multilabel, a row otherwise), 256
words per block of the pack kernel, byte fields four to a word.  C = 3 with shards of one row puts the byte destinations
at every residue mod 4; a shard of 301 rows x 13 classes takes 16 blocks and ends inside one; empty shards, first ones
included, launch blocks that do nothing."""
import ctypes as C

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_cases as ec  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import _lib, metrics, ops  # noqa: E402

DEV = "cuda"
T = torch.from_numpy
STORE = ("_score", "_pred", "_label", "_predict", "_raw", "_target")


def inputs(kind, N, Cn):
    """Grid logits (ties), both zeros, and targets the kernels refuse."""
    tag = f"shard.{kind}.{N}.{Cn}."
    if kind == "multilabel":
        x = ec.grid_logits(tag + "x", (N, Cn))
        y = (ec.det(tag + "y", (N, Cn)) < -0.5244).astype(np.float32)
        x.flat[0], x.flat[1] = 0.0, -0.0
        y.flat[2], y.flat[N * Cn - 1] = 0.5, np.nan
        return x, y
    if kind == "regression":
        x = ec.grid_logits(tag + "x", (N,))
        x[0], x[N - 1] = -0.0, 0.0                                # raw keeps the sign bit
        y = (np.clip(np.rint(ec.det(tag + "y", (N,)).astype(np.float64) * 6), -12, 12) / 4).astype(np.float32)
        return x, y
    x = ec.grid_logits(tag + "x", (N, Cn))
    y = (np.abs(ec.det(tag + "y", (N,))) * 1.7).astype(np.int64) % Cn
    y[0], y[N - 1] = -1, Cn
    return x, y


def spans_of(shard_rows, bs):
    """Per shard, the (lo, hi) row spans of its batches in the global order."""
    out, r0 = [], 0
    for n in shard_rows:
        out.append([(r0 + lo, r0 + hi) for lo, hi in ec.batches_of(n, bs)])
        r0 += n
    return out


GATE_WIDTH = 5
GATE_DTYPE = {"multilabel": torch.float16, "regression": torch.float32, "classes": torch.float64}


def gates_of(kind, N):
    """Gates [N, 5] in a dtype per kind (2, 4 and 8 bytes: rows of 10, 20 and 40 bytes), a negative zero among them."""
    g = ec.det(f"shard.{kind}.{N}.gates", (N, GATE_WIDTH)).astype(np.float64)
    g[0, 0] = -0.0
    return T(g).to(GATE_DTYPE[kind]).to(DEV)


def feed(ev, x, y, spans, first_batch, with_losses, gates=None):
    for i, (lo, hi) in enumerate(spans):
        loss = torch.tensor(0.125 * (first_batch + i) - 0.5, dtype=torch.float32, device=DEV) if with_losses else None
        ev.update(T(np.ascontiguousarray(x[lo:hi])).to(DEV), T(np.ascontiguousarray(y[lo:hi])).to(DEV), loss,
                  None if gates is None else gates[lo:hi])


def bits(t):
    return t.view(torch.int32) if t.dtype == torch.float32 else t


def assert_store_equal(a, b, N, nb):
    assert (a.n, a.nbatches, a.nlosses) == (b.n, b.nbatches, b.nlosses) == (N, nb, b.nlosses)
    for name in STORE:
        ta, tb = getattr(a, name), getattr(b, name)
        assert (ta is None) == (tb is None), name
        if ta is not None:
            assert torch.equal(bits(ta[:N]), bits(tb[:N])), name
    assert torch.equal(bits(a._losses[:nb]), bits(b._losses[:nb]))
    assert torch.equal(a._bad, b._bad)


def same(a, b):
    """== on every number and array of two compute() dicts, NaN equal to NaN."""
    if isinstance(a, dict):
        return isinstance(b, dict) and set(a) == set(b) and all(same(a[k], b[k]) for k in a)
    return np.array_equal(np.asarray(a), np.asarray(b), equal_nan=True)


def snapshot(ev):
    return [None if getattr(ev, n) is None else getattr(ev, n).clone() for n in STORE] + [ev._losses.clone(), ev._out.clone()], \
        (ev.n, ev.nbatches, ev.nlosses)


def assert_unchanged(ev, snap):
    tensors, counts = snap
    now, counts_now = snapshot(ev)
    assert counts_now == counts
    for a, b in zip(now, tensors):
        assert (a is None and b is None) or torch.equal(a.view(torch.uint8), b.view(torch.uint8))


def run_case(kind, Cn, shard_rows, with_losses, into_source=None, bs=3):
    N, W = sum(shard_rows), len(shard_rows)
    x, y = inputs(kind, N, Cn)
    spans = spans_of(shard_rows, bs)
    nbs = [len(s) for s in spans]
    nb = sum(nbs)
    ref = metrics.Evaluator(kind, Cn, N + 3, max_batches=nb + 1, device=DEV)
    gates = gates_of(kind, N)
    feed(ref, x, y, [s for sh in spans for s in sh], 0, with_losses, gates)
    shards, b0 = [], 0
    for r, sh in enumerate(spans):
        big = r == into_source
        ev = metrics.Evaluator(kind, Cn, N + 3 if big else max(shard_rows[r], 1), max_batches=nb + 1 if big else max(nbs[r], 1), device=DEV)
        feed(ev, x, y, sh, b0, with_losses, gates)
        b0 += nbs[r]
        shards.append(ev)
    losses = nbs if with_losses else [0] * W
    images = torch.stack([ev.pack(max(shard_rows), max(losses)) for ev in shards])
    dest = shards[into_source] if into_source is not None else metrics.Evaluator(kind, Cn, N + 3, max_batches=nb + 1, device=DEV)
    # the gates travel beside the images, as all_gather moves them: a slot of bytes per shard, laid out in shard order
    slots = torch.zeros((W, metrics.Evaluator.gate_slot_bytes(max(shard_rows), GATE_WIDTH, GATE_DTYPE[kind])), dtype=torch.uint8, device=DEV)
    for ev, slot in zip(shards, slots):
        ev.pack_gates(slot)
    dest.merge(images, shard_rows, nbs, losses)
    dest.merge_gates(slots, shard_rows, GATE_WIDTH, GATE_DTYPE[kind])
    assert_store_equal(dest, ref, N, nb)
    got, want = dest.compute(), ref.compute()
    assert same(got, want), (got, want)
    assert want["bad"] == (0 if kind == "regression" else 2) and (np.isnan(want["loss"]) != with_losses)
    assert len(ref.predictions()) == 4 and ref.predictions()[3].shape == (N, GATE_WIDTH)
    for a, b in zip(dest.predictions(), ref.predictions()):
        assert (a is None and b is None) or (a.dtype == b.dtype and np.array_equal(a.view(np.uint8), b.view(np.uint8)))


KINDS = [("multilabel", 3), ("multilabel", 13), ("regression", 1), ("classes", 3), ("classes", 13)]
SHARDS = [[6], [3, 4], [5, 0, 7], [0, 4, 3], [1, 1, 1, 1, 1, 1, 1, 2]]


@pytest.mark.parametrize("shard_rows", SHARDS, ids=lambda s: "-".join(map(str, s)))
@pytest.mark.parametrize("kind,Cn", KINDS)
def test_merged_shards_equal_the_unsharded_store(kind, Cn, shard_rows):
    run_case(kind, Cn, shard_rows, with_losses=True)


@pytest.mark.parametrize("kind,Cn", [("multilabel", 13), ("regression", 1), ("classes", 13)])
def test_many_blocks_per_shard(kind, Cn):
    """301 rows x 13 classes: 16 blocks of the merge kernel for the first shard, the last one partly filled; the next shard
    starts at element 3913 (residue 1 mod 4)."""
    run_case(kind, Cn, [301, 2, 40], with_losses=True, bs=128)


@pytest.mark.parametrize("kind,Cn", [("multilabel", 3), ("regression", 1), ("classes", 3)])
def test_without_losses(kind, Cn):
    run_case(kind, Cn, [5, 0, 7], with_losses=False)


@pytest.mark.parametrize("kind,Cn", [("multilabel", 3), ("regression", 1), ("classes", 13)])
@pytest.mark.parametrize("source", [0, 2])
def test_merge_into_a_store_whose_image_is_a_source(kind, Cn, source):
    run_case(kind, Cn, [3, 4, 2], with_losses=True, into_source=source)


def test_image_is_a_function_of_the_shard():
    """Every word is written, zero past the shard's data, whatever the buffer held; a sum of images that are zero outside
    their own slot (what the all-reduce does) reproduces each."""
    x, y = inputs("multilabel", 7, 3)
    ev = metrics.Evaluator("multilabel", 3, 16, device=DEV)
    feed(ev, x, y, [(0, 3), (3, 7)], 0, True)
    tight = ev.pack()
    assert tight.dtype == torch.int32 and tight.numel() * 4 == ops.eval_image_bytes(metrics.KINDS["multilabel"], 7, 2, 3)
    wide = ev.pack(11, 5)
    dirty = ev.pack(11, 5, out=torch.full((wide.numel() + 9,), -1, dtype=torch.int32, device=DEV))
    assert torch.equal(dirty[:wide.numel()], wide) and not dirty[wide.numel():].any()
    w = wide.cpu().numpy()
    assert w[0] == 2 and w[1] == 0 and w[2:4].all() and not w[4:7].any()   # bad, void mark, 2 losses, losses [2, 5): zero
    score = w[7:7 + 33].view(np.float32)
    assert np.array_equal(score[:21], ec.sigmoid32(x).ravel()) and not w[7 + 21:7 + 33].any()
    empty = metrics.Evaluator("multilabel", 3, 1, device=DEV).pack(11, 5)
    assert not empty.any()
    slots = torch.zeros((3, wide.numel()), dtype=torch.int32, device=DEV)
    slots[1] = wide
    assert torch.equal(slots.sum(0, dtype=torch.int32), wide)
    with pytest.raises(ValueError, match="pack"):
        ev.pack(6, 2)


def test_pack_and_merge_do_not_synchronise():
    x, y = inputs("classes", 9, 3)
    a, b = metrics.Evaluator("classes", 3, 16, device=DEV), metrics.Evaluator("classes", 3, 16, device=DEV)
    feed(a, x, y, [(0, 5)], 0, True)
    feed(b, x, y, [(5, 9)], 1, True)
    images = torch.empty((2, ops.eval_image_bytes(metrics.KINDS["classes"], 5, 1, 3) // 4), dtype=torch.int32, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        a.pack(5, 1, out=images[0])
        b.pack(5, 1, out=images[1])
        a.merge(images, [5, 4], [1, 1])
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    ref = metrics.Evaluator("classes", 3, 16, device=DEV)
    feed(ref, x, y, [(0, 5), (5, 9)], 0, True)
    assert_store_equal(a, ref, 9, 2)


def test_refusals_leave_the_destination_unchanged():
    kind, Cn = "multilabel", 3
    x, y = inputs(kind, 12, Cn)
    a, b = metrics.Evaluator(kind, Cn, 8, device=DEV), metrics.Evaluator(kind, Cn, 8, device=DEV)
    feed(a, x, y, [(0, 3), (3, 5)], 0, True)
    feed(b, x, y, [(5, 9)], 2, True)
    images = torch.stack([a.pack(5, 2), b.pack(5, 2)])
    dest = metrics.Evaluator(kind, Cn, 10, max_batches=4, device=DEV)
    feed(dest, x, y, [(8, 12)], 0, True)
    snap = snapshot(dest)
    short = images[:, :images.shape[1] - 1].contiguous()
    for bad_images, rows, batches, what in (
            (images, [5, 6], [2, 1], "capacity"),                 # 11 rows into a capacity of 10
            (images, [5, 4], [2, 3], "max_batches"),              # 5 batches of at most 4
            (short, [5, 4], [2, 1], "images"),                    # one word short of the layout for (5 rows, 2 losses)
            (images, [5, -1], [2, 1], "negative"),
            (images, [5, 4], [2, -1], "negative"),
            (images, [5, 4, 0], [2, 1, 0], "images")):            # three shards, two images
        with pytest.raises(ValueError, match=what):
            dest.merge(bad_images, rows, batches)
        assert_unchanged(dest, snap)
        if len(rows) == bad_images.shape[0]:                      # the C entry point refuses on its own: BPM_ERR_ARG
            with pytest.raises(RuntimeError, match=r"bpm_eval_merge failed \(code -1\)"):
                ops.eval_merge(dest._desc, bad_images, rows, batches)
            assert_unchanged(dest, snap)
    with pytest.raises(ValueError, match="loss"):
        dest.merge(images, [5, 4], [2, 1], [2, 0])                # losses for some batches only
    with pytest.raises(RuntimeError, match=r"bpm_eval_pack failed \(code -1\)"):
        ops.eval_pack(dest._desc, 4, 1, torch.zeros(8, dtype=torch.int32, device=DEV))          # an image that is too small
    with pytest.raises(RuntimeError, match=r"bpm_eval_pack failed \(code -1\)"):
        ops.eval_pack(dest._desc, -1, 1, torch.zeros(64, dtype=torch.int32, device=DEV), rows=4)
    room = torch.zeros(64, dtype=torch.int32, device=DEV)
    lib = _lib.lib()                                               # misaligned pointers: BPM_ERR_ALIGN, nothing launched
    assert lib.bpm_eval_pack(C.byref(dest._desc), 4, 1, 4, 1, room.data_ptr() + 2, 84, None) == -2
    assert lib.bpm_eval_merge(C.byref(dest._desc), images.data_ptr() + 2, images.shape[1] * 4, 2, (C.c_int * 2)(5, 4), (C.c_int * 2)(2, 1),
                              None) == -2
    assert lib.bpm_eval_merge(C.byref(dest._desc), images.data_ptr(), images.shape[1] * 4, 65, None, None, None) == -1
    assert ops.eval_image_bytes(7, 4, 1, 3) == 0 and ops.eval_image_bytes(metrics.KINDS[kind], -1, 1, 3) == 0
    assert_unchanged(dest, snap)
    void = images.clone()
    void[1, 1] = 1                                                # a voided shard: the merge leaves bad = -1, compute() raises
    other = metrics.Evaluator(kind, Cn, 10, device=DEV)
    other.merge(void, [5, 4], [2, 1])
    assert int(other._bad[0].cpu()) == -1
    with pytest.raises(ValueError, match="voided"):
        other.compute()
    dest.merge(images, [5, 4], [2, 1])                            # and the same call with honest counts goes through
    ref = metrics.Evaluator(kind, Cn, 10, device=DEV)
    feed(ref, x, y, [(0, 3), (3, 5), (5, 9)], 0, True)
    assert_store_equal(dest, ref, 9, 3)
