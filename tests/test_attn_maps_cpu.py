"""Attention maps without a GPU.

1. The fixture F16 (tests/golden/make_golden_attn_maps.py: the reference's head-averaged attention weights) against what
   can be derived without the reference: every stored full map has rows that sum to 1 within S * 2^-23 (an fp32 softmax
   row sums to 1 within about one rounding per term; the head average keeps that) and is exactly 0 at the keys the future
   mask hides, j - i >= 1 + |S - T|; the stored rows of the whole-model maps likewise.
2. Host logic (ops._DRY_RUN): the launch table `attention_maps()` builds for a crossmodal, a self-only and a biprojection
   plan -- one problem per encoder x layer x block, reading the plan's qh / kh / lse (qs / ks / lses for the self half of a
   biprojection layer) with the forward problem's mask_off and q_pos0 / q_stride -- for the model's two schedules, and
   the error paths (before a forward, unknown encoder, layer out of range).
3. The C ABI entry validates its arguments on the host."""
import ctypes as C
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, engine, ops
from bpmult_amd.models import get_model
from bpmult_amd.models.encoder import TransformerEncoder

G = os.path.join(os.path.dirname(__file__), "golden")

# (case, T, S, layers, blocks, attn_mask): the standalone cases of F16
STANDALONE = [("x", 7, 5, 2, ("cross",), True), ("xn", 6, 6, 2, ("cross",), False), ("x25", 8, 11, 2, ("cross",), True),
              ("b", 5, 8, 2, ("self", "cross"), True),
              ("sb", 7, 7, 2, ("self",), True), ("sn", 9, 9, 2, ("self",), False), ("s25", 70, 70, 2, ("self",), True),
              ("s128", 130, 130, 2, ("self",), True), ("s256", 40, 40, 1, ("self",), True),
              ("c130x70", 130, 70, 2, ("cross",), True), ("c70x130", 70, 130, 2, ("cross",), True),
              ("c128", 70, 40, 1, ("cross",), True), ("c256", 40, 70, 1, ("self", "cross"), True)]


@pytest.fixture(scope="module")
def f16():
    return dict(np.load(os.path.join(G, "f16_attn_maps.npz")))


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    del ops._DRY_LAUNCHES[:]
    try:
        yield
    finally:
        ops._DRY_RUN = False
        del ops._DRY_LAUNCHES[:]


@pytest.mark.parametrize("tag,Tn,S,L,blocks,mask", STANDALONE, ids=[c[0] for c in STANDALONE])
def test_fixture_maps_are_row_stochastic_and_masked(f16, tag, Tn, S, L, blocks, mask):
    n = 0
    for i in range(L):
        for blk in blocks:
            w = f16[f"{tag}.L{i}.{blk}"]
            Sk = Tn if blk == "self" else S
            assert w.shape == (2, Tn, Sk) and w.dtype == np.float32
            assert np.isfinite(w).all() and (w >= 0).all()
            err = np.abs(w.astype(np.float64).sum(-1) - 1.0).max()
            assert err <= Sk * 2.0 ** -23, (tag, i, blk, err)
            if mask:
                ii, jj = np.arange(Tn)[:, None], np.arange(Sk)[None, :]
                hidden = (jj - ii) >= 1 + abs(Sk - Tn)
                assert (w[:, hidden] == 0).all(), (tag, i, blk)
                assert (w[:, ~hidden] > 0).all(), (tag, i, blk)
            n += 1
    assert n == L * len(blocks)
    assert not any(k.startswith(f"{tag}.L{L}.") for k in f16)


def test_fixture_model_rows(f16):
    names = f16["m.names"].tolist()
    rows = f16["m.query_rows"]
    assert len(names) == 12 and rows.tolist() == [0, 1, 63, 64, 255, 256, 510, 511]
    for n in names:
        for i in range(2):
            w = f16[f"m.{n}.L{i}.rows"]
            assert w.shape == (2, 8, 512)
            assert np.abs(w.astype(np.float64).sum(-1) - 1.0).max() <= 512 * 2.0 ** -23
            hidden = (np.arange(512)[None, :] - rows[:, None]) >= 1
            assert (w[:, hidden] == 0).all() and (w[:, ~hidden] > 0).all()
            nrm, tot = f16[f"m.{n}.L{i}.n"]
            assert abs(tot - 2 * 512) <= 2 * 512 * 512 * 2.0 ** -23 and 0 < nrm <= (2 * 512) ** 0.5 + 1e-6   # rows sum to 1; |row|_2 <= 1


def _problems(launches):
    out = []
    for fn, dtype, arr in launches:
        assert fn is ops.attn_maps
        out += [(dtype, p) for p in arr]
    return out


def _same_rule(p, a, Q, K, lse):
    """Map problem p reads the buffers of forward problem a with its visibility rule."""
    assert (p.Q, p.K, p.lse) == (Q.data_ptr(), K.data_ptr(), lse.data_ptr()) == (a.Q, a.K, a.lse)
    assert (p.B, p.H, p.T, p.S, p.dh, p.dhp) == (a.B, a.H, a.T, a.S, a.dh, a.dhp)
    assert (p.mask_off, p.q_pos0, p.q_stride) == (a.mask_off, a.q_pos0, a.q_stride)
    assert p.ldw == p.S and p.W


def _fwd_attn(plan):
    """Forward attention problems of the plan by their lse pointer."""
    un = lambda s: s[1] if isinstance(s, tuple) and s[0] in (engine.SIDE, engine.SIDE2) else s
    out = {}
    for s in plan._fwd[False]:
        if s is engine.JOIN or not callable(un(s)[0]):
            continue
        s = un(s)
        if s[0] is ops.attn_fwd:
            for a in s[2]:
                out[a.lse] = a
    return out


@pytest.mark.parametrize("prec", ["bf16", "f32", "bf16x3"])
@pytest.mark.parametrize("kind", ["cross", "self", "biprojection"])
def test_standalone_plan_tables(dry_run, kind, prec):
    d, H, L, B, Tn, S = 24, 4, 3, 2, 7, 9
    enc = TransformerEncoder(d, H, L, attn_mask=True, biprojection=kind == "biprojection")
    enc.precision = prec
    enc._ensure_store()
    with pytest.raises(RuntimeError, match="forward"):
        enc.attention_maps()
    x, kv = torch.zeros(Tn, B, d), torch.zeros(S, B, d)
    plan = enc._plan_for(x, None if kind == "self" else kv)
    with pytest.raises(RuntimeError, match="forward"):
        plan.attention_maps()
    plan.maps_ready()                          # what a finished forward leaves (nothing can run here)
    enc._last_plan = plan
    maps = enc.attention_maps()
    (b,) = plan.buf
    fwd = _fwd_attn(plan)
    blocks = {"cross": ("cross",), "self": ("self",), "biprojection": ("self", "cross")}[kind]
    assert len(maps) == L and all(tuple(m) == blocks for m in maps)
    probs = _problems(ops._DRY_LAUNCHES)
    assert len(probs) == L * len(blocks) and all(dt == plan.dtype for dt, _ in probs)
    k = 0
    for i in range(L):
        for blk in blocks:
            p = probs[k][1]
            k += 1
            if blk == "self":
                keys = ("qh", "kh", "lse") if kind == "self" else ("qs", "ks", "lses")
            else:
                keys = ("qh", "kh", "lse")
            Q, K, lse = (b[n][i] for n in keys)
            _same_rule(p, fwd[lse.data_ptr()], Q, K, lse)
            m = maps[i][blk]
            assert m.query_steps is None and m.weights.shape == (B, Tn, Tn if blk == "self" else S)
            assert m.weights.dtype == torch.float32 and m.weights.is_contiguous() and p.W == m.weights.data_ptr()
    del ops._DRY_LAUNCHES[:]
    sel = enc.attention_maps(layers=[2, 0])
    assert len(sel) == 2 and len(_problems(ops._DRY_LAUNCHES)) == 2 * len(blocks)
    assert _problems(ops._DRY_LAUNCHES)[0][1].lse == b["lses" if kind == "biprojection" else "lse"][2].data_ptr()
    for bad in ([L], [-1], ["0"]):
        with pytest.raises(IndexError):
            enc.attention_maps(layers=bad)
    with pytest.raises(ValueError, match="no encoder"):
        plan.attention_maps(encoders=["nope"])
    with pytest.raises(IndexError):
        plan.attention_maps(encoders=[1])


def _args(model, **kw):
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=64, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1, res_dropout=0.1,
             out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=40, num_vectors_v=40)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("model", ["mmtrvat", "mmtrvapt"])
def test_model_tables(dry_run, model, prune):
    from bpmult_amd.models.bpmult import ENC_ORDER, LEVEL1, LEVEL2
    m = get_model(_args(model, prune_unused_rows=prune, **({"orig_d_a": 96} if model == "mmtrvapt" else {})))
    m._ensure_store()
    with pytest.raises(RuntimeError, match="forward"):
        m.attention_maps()
    B, L = 2, m.layers
    trunk = m._trunk_for(B)
    trunk.plan1.maps_ready()
    trunk.plan2.maps_ready()
    m._last_trunk = trunk
    maps = m.attention_maps()
    assert list(maps) == ENC_ORDER and all(len(v) == L for v in maps.values())
    four = model == "mmtrvapt"
    N = trunk.N
    nprob = 0
    for plan, level in ((trunk.plan1, LEVEL1), (trunk.plan2, LEVEL2)):
        fwd = _fwd_attn(plan)
        for (name, spec), e, b in zip(level.items(), plan.encs, plan.buf):
            Tfull = N[spec[0]]
            for i in range(L):
                got = maps[name][i]
                assert tuple(got) == (("self", "cross") if (four and level is LEVEL2) else ("cross",))
                nprob += len(got)
                few = prune and level is LEVEL2 and (not four or i == L - 1)
                for blk, mp in got.items():
                    Sk = Tfull if blk == "self" else e.S
                    assert mp.weights.shape == (B, 2 if few else Tfull, Sk)
                    assert mp.query_steps == ((0, Tfull - 1) if few else None)
                    keys = ("qs", "ks", "lses") if blk == "self" else ("qh", "kh", "lse")
                    Q, K, lse = (b[n][i] for n in keys)
                    p = next(p for _, p in _problems(ops._DRY_LAUNCHES) if p.W == mp.weights.data_ptr())
                    _same_rule(p, fwd[lse.data_ptr()], Q, K, lse)
                    if few:
                        assert (p.T, p.q_pos0, p.q_stride) == (2, 0, Tfull - 1)
    assert len(_problems(ops._DRY_LAUNCHES)) == nprob
    # selection: nothing is built for what is not asked for
    del ops._DRY_LAUNCHES[:]
    sel = m.attention_maps(names=["trans_l_with_v2a", "trans_v_with_a"], layers=[1])
    assert list(sel) == ["trans_l_with_v2a", "trans_v_with_a"] and all(len(v) == 1 for v in sel.values())
    assert len(_problems(ops._DRY_LAUNCHES)) == (3 if four else 2)
    with pytest.raises(ValueError, match="unknown encoder"):
        m.attention_maps(names=["trans_l_with_l"])
    with pytest.raises(IndexError):
        m.attention_maps(layers=[L])
    m.set_prune_unused_rows(not prune)             # drops the activation buffers
    with pytest.raises(RuntimeError, match="forward"):
        m.attention_maps()


def test_entry_validates_its_arguments():
    _lib.build()
    L = _lib.lib()
    p = _lib.AttnMapProblem()
    assert L.bpm_attn_maps(_lib.BPM_F32, C.byref(p), 1, None) == -1              # all-zero problem
    assert L.bpm_attn_maps(_lib.BPM_F32, C.byref(p), 0, None) == -1
    assert L.bpm_attn_maps(_lib.BPM_F32, None, 1, None) == -1
    p.Q, p.K, p.lse, p.W = 64, 128, 256, 512
    p.B, p.H, p.T, p.S, p.dh, p.dhp, p.ldw = 1, 2, 5, 7, 25, 32, 6
    assert L.bpm_attn_maps(_lib.BPM_BF16, C.byref(p), 1, None) == -1             # ldw < S
    p.ldw = 7
    p.dh = 40
    assert L.bpm_attn_maps(_lib.BPM_BF16, C.byref(p), 1, None) == -1             # dh > dhp
    p.dh, p.dhp = 25, 48
    assert L.bpm_attn_maps(_lib.BPM_BF16, C.byref(p), 1, None) == -1             # dhp not an instantiation
    p.dhp = 32
    assert L.bpm_attn_maps(3, C.byref(p), 1, None) == -1                          # dtype
    p.Q = 72
    assert L.bpm_attn_maps(_lib.BPM_BF16, C.byref(p), 1, None) == -2             # Q not 16-byte aligned
    p.Q, p.W = 64, 514
    assert L.bpm_attn_maps(_lib.BPM_BF16, C.byref(p), 1, None) == -2             # W not 4-byte aligned
    p.W = 512
    p.q_stride = -1
    assert L.bpm_attn_maps(_lib.BPM_BF16, C.byref(p), 1, None) == -1
    arr = (_lib.AttnMapProblem * (_lib.MAX_GROUP + 1))()
    assert L.bpm_attn_maps(_lib.BPM_BF16, arr, _lib.MAX_GROUP + 1, None) == -1   # group size
    assert _lib.PROF_KINDS["attn_maps"] == 16
