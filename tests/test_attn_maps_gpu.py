"""Head-averaged attention maps on the MI355X (bpm_attn_maps, EncoderGroupPlan.attention_maps and the module surface).

1. The kernel through the C ABI against float64 torch from the same rounded Q / K (softmax in float64), LSE taken from
   bpm_attn_fwd on the same inputs.  Limits: tests/test_kernels_gpu.py's `tol()` for the forward output in the same dtype
   (f32 2e-5, bf16 1.5e-2); probabilities are <= 1, so they act as absolute limits.  Masked entries compare == 0.
2. The reference's maps (fixture F16, tests/golden/make_golden_attn_maps.py) through TransformerEncoder.forward +
   attention_maps() in f32, bf16x3 and bf16, and through the 3-modal model in both schedules, eager and graph replay.
   f32: 2e-4 (scale 1: the limit test_encoder_gpu.py::test_f5_encoder holds y to on these cases).  bf16 / bf16x3: max-abs
   and relative-L2 error per case, <= 2x the errors measured on the MI355X (MEASURED below;
   profiles/r06_attn_maps_errors.json, written through BPMULT_ERROR_LOG).
3. Properties that need no reference, and: taking the maps does not disturb the training step."""
import copy
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detgen import det, det_param  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import ops  # noqa: E402
from bpmult_amd._lib import BPM_BF16, BPM_F32  # noqa: E402
from bpmult_amd.engine import dhp_for  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.models.encoder import TransformerEncoder  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
DEV = "cuda"
B = 2


def tol(dtype):                      # == tests/test_kernels_gpu.py:tol
    return 2e-5 if dtype == BPM_F32 else 1.5e-2


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------------
# 1. kernel
# ---------------------------------------------------------------------------------------------------------------------
def _kernel_problem(dtype, Bn, H, Tn, S, dh, masked, qpos=None, ldw=None, seed=0):
    """Random Q / K / V in the head-major padded layout, LSE by bpm_attn_fwd; returns (map problem, W, float64 reference,
    hidden-key mask, tensors to keep alive)."""
    dhp, ctt = dhp_for(dh), ops.ct_torch(dtype)
    ld = ops.pad32(H * dh)

    def heads(x):
        buf = torch.zeros(*x.shape[:3], dhp, dtype=ctt)
        buf[..., :dh] = x.to(ctt)
        return buf.to(DEV), buf[..., :dh].double()

    Q, q = heads(rnd(Bn, H, Tn, dh, seed=31 + seed) * dh ** -0.5 * 2.0)
    K, k = heads(rnd(Bn, H, S, dh, seed=32 + seed) * 1.5)
    V, _ = heads(rnd(Bn, H, S, dh, seed=33 + seed))
    p0, st = qpos if qpos is not None else (0, 1)
    Tfull = p0 + (Tn - 1) * st + 1
    off = 1 + abs(S - Tfull) if masked else 0
    O = torch.zeros(Tn * Bn, ld, device=DEV, dtype=ctt)
    lse = torch.zeros(Bn, H, Tn, device=DEV)
    ops.attn_fwd(dtype, [ops.attn_problem(Q, K, V, O, ld, lse, Bn, H, Tn, S, dh, dhp, off, q_pos0=p0, q_stride=st)])
    s = q @ k.transpose(-1, -2)
    hidden = torch.zeros(Tn, S, dtype=torch.bool)
    if masked:
        i = p0 + st * torch.arange(Tn)[:, None]
        hidden = (torch.arange(S)[None, :] - i) >= off
        s = s.masked_fill(hidden, float("-inf"))
    ref = torch.softmax(s, -1).mean(1)
    ldw = S if ldw is None else ldw
    W = torch.full((Bn, Tn, ldw), 7.0, device=DEV)
    p = ops.attn_map_problem(Q, K, lse, W, ldw, Bn, H, Tn, S, dh, dhp, off, q_pos0=p0, q_stride=st)
    return p, W, ref, hidden, (Q, K, V, O, lse)


def _check_kernel(W, ref, hidden, dtype, S, what):
    torch.cuda.synchronize()
    got = W[..., :S].double().cpu()
    assert torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} (limit {tol(dtype):.1e})")
    assert (got[:, hidden] == 0).all(), what + ": masked entries must be exactly 0"
    assert err <= tol(dtype), f"{what}: max err {err:.3e} > {tol(dtype):.1e}"
    assert (W[..., S:] == 7.0).all(), what + ": pad columns were written"


KERNEL_SHAPES = [(2, 3, 70, 100, 25, True, None), (2, 2, 100, 70, 6, True, None), (1, 2, 130, 130, 64, True, None),
                 (1, 2, 513, 512, 25, True, None), (1, 12, 512, 512, 64, True, None), (1, 2, 2, 200, 25, True, (0, 199)),
                 (3, 2, 2, 72, 64, True, (0, 71)), (1, 1, 33, 65, 64, False, None), (2, 3, 70, 100, 25, False, None),
                 (1, 2, 200, 512, 128, True, None), (1, 2, 512, 200, 128, True, None), (1, 6, 50, 50, 128, True, None),
                 (1, 2, 70, 130, 256, True, None), (2, 1, 130, 70, 200, True, None), (1, 2, 2, 130, 256, True, (0, 129)),
                 (1, 1, 1, 1, 25, True, None)]


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("Bn,H,Tn,S,dh,masked,qpos", KERNEL_SHAPES)
def test_kernel_against_float64(dtype, Bn, H, Tn, S, dh, masked, qpos):
    p, W, ref, hidden, keep = _kernel_problem(dtype, Bn, H, Tn, S, dh, masked, qpos, ldw=S + 5 if S % 2 else None)
    ops.attn_maps(dtype, [p])
    _check_kernel(W, ref, hidden, dtype, S, f"{Bn}x{H}x{Tn}x{S} dh {dh}")


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16], ids=["f32", "bf16"])
@pytest.mark.parametrize("dh", [25, 64, 128, 256])
def test_kernel_grouped_launch_and_padded_rows(dtype, dh):
    """Several problems of different shapes in one launch (more than BPM_MAX_GROUP: two launches), ldw > S."""
    shapes = [(2, 3, 70, 100, True, None, 104), (1, 2, 130, 64, True, None, 64), (2, 2, 2, 96, True, (0, 95), 128),
              (1, 1, 65, 65, False, None, 70), (1, 4, 7, 5, True, None, 5)]
    shapes = shapes * 4                                  # 20 problems
    made = [_kernel_problem(dtype, Bn, H, Tn, S, dh, m, qp, ldw=ldw, seed=7 * n) for n, (Bn, H, Tn, S, m, qp, ldw) in enumerate(shapes)]
    ops.attn_maps(dtype, [m[0] for m in made])
    for n, ((p, W, ref, hidden, keep), sh) in enumerate(zip(made, shapes)):
        _check_kernel(W, ref, hidden, dtype, sh[3], f"problem {n} {sh}")


# ---------------------------------------------------------------------------------------------------------------------
# 2. the reference's maps (F16)
# ---------------------------------------------------------------------------------------------------------------------
# (case, weights prefix, biprojection, d, heads, layers, T, S (0: forward(x)), attn_mask)
CASES = [("x", "f5x.", False, 24, 4, 2, 7, 5, True), ("xn", "f5xn.", False, 24, 4, 2, 6, 6, False),
         ("x25", "f5x25.", False, 50, 2, 2, 8, 11, True), ("b", "f5b.", True, 24, 4, 2, 5, 8, True),
         ("sb", "f15sb.", True, 24, 4, 2, 7, 0, True), ("sn", "f15sn.", False, 24, 4, 2, 9, 0, False),
         ("s25", "f15s25.", False, 50, 2, 2, 70, 0, True), ("s128", "f15s128.", False, 256, 2, 2, 130, 0, True),
         ("s256", "f15s256.", True, 512, 2, 1, 40, 0, True),
         ("c130x70", "f16c130x70.", False, 50, 2, 2, 130, 70, True), ("c70x130", "f16c70x130.", False, 50, 2, 2, 70, 130, True),
         ("c128", "f16c128.", False, 256, 2, 1, 70, 40, True), ("c256", "f16c256.", True, 512, 2, 1, 40, 70, True)]
F32_LIMIT = 2e-4
# Largest max-abs / relative-L2 error of a case's maps against F16, measured on the MI355X (rounded up to two digits;
# profiles/r06_attn_maps_errors.json); the limits are 2x these.
MEASURED = {
    "bf16.b": {"max_abs": 2.2e-03, "rel_l2": 3.0e-03},
    "bf16.c128": {"max_abs": 3.3e-04, "rel_l2": 1.6e-03},
    "bf16.c130x70": {"max_abs": 3.8e-04, "rel_l2": 1.6e-03},
    "bf16.c256": {"max_abs": 1.6e-02, "rel_l2": 1.2e-02},
    "bf16.c70x130": {"max_abs": 1.9e-04, "rel_l2": 1.7e-03},
    "bf16.s128": {"max_abs": 9.0e-04, "rel_l2": 1.3e-03},
    "bf16.s25": {"max_abs": 6.4e-04, "rel_l2": 1.2e-03},
    "bf16.s256": {"max_abs": 7.0e-04, "rel_l2": 1.2e-03},
    "bf16.sb": {"max_abs": 7.0e-04, "rel_l2": 8.9e-04},
    "bf16.sn": {"max_abs": 4.4e-04, "rel_l2": 1.2e-03},
    "bf16.x": {"max_abs": 5.5e-04, "rel_l2": 7.8e-04},
    "bf16.x25": {"max_abs": 5.9e-04, "rel_l2": 1.4e-03},
    "bf16.xn": {"max_abs": 9.6e-04, "rel_l2": 9.6e-04},
    "bf16x3.b": {"max_abs": 2.4e-07, "rel_l2": 2.6e-07},
    "bf16x3.c128": {"max_abs": 6.0e-08, "rel_l2": 2.9e-07},
    "bf16x3.c130x70": {"max_abs": 4.5e-08, "rel_l2": 2.8e-07},
    "bf16x3.c256": {"max_abs": 4.0e-06, "rel_l2": 2.8e-06},
    "bf16x3.c70x130": {"max_abs": 3.8e-08, "rel_l2": 3.0e-07},
    "bf16x3.s128": {"max_abs": 1.2e-07, "rel_l2": 2.1e-07},
    "bf16x3.s25": {"max_abs": 9.0e-08, "rel_l2": 1.7e-07},
    "bf16x3.s256": {"max_abs": 1.2e-07, "rel_l2": 2.2e-07},
    "bf16x3.sb": {"max_abs": 9.0e-08, "rel_l2": 8.2e-08},
    "bf16x3.sn": {"max_abs": 4.5e-08, "rel_l2": 1.3e-07},
    "bf16x3.x": {"max_abs": 6.0e-08, "rel_l2": 1.2e-07},
    "bf16x3.x25": {"max_abs": 1.2e-07, "rel_l2": 1.7e-07},
    "bf16x3.xn": {"max_abs": 6.0e-08, "rel_l2": 1.4e-07},
}

_FIX = {}
_MEAS = {}
# where the measured errors go (the JSON of profiles/r06_attn_maps_errors.json): set BPMULT_ERROR_LOG to a file path to
# record them; unset, nothing is written
_LOG = os.environ.get("BPMULT_ERROR_LOG")


def load(name):
    if name not in _FIX:
        _FIX[name] = dict(np.load(os.path.join(G, name + ".npz")))
    return _FIX[name]


def _note(prec, tag, max_abs, rel):
    key = f"{prec}.{tag}"
    old = _MEAS.get(key, {"max_abs": 0.0, "rel_l2": 0.0})
    _MEAS[key] = {"max_abs": max(old["max_abs"], max_abs), "rel_l2": max(old["rel_l2"], rel)}
    if not _LOG:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(_LOG)), exist_ok=True)
        with open(_LOG, "w") as f:
            json.dump(_MEAS, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _errors(got, ref):
    a, b = got.detach().double().cpu().numpy(), ref.astype(np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all()
    return float(np.abs(a - b).max()), float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))


def _hidden(Tn, S, mask):
    if not mask:
        return np.zeros((Tn, S), dtype=bool)
    return (np.arange(S)[None, :] - np.arange(Tn)[:, None]) >= 1 + abs(S - Tn)


def _inputs(pfx, what, n, d):
    x = T(det(pfx + what, (n, B, d)))
    m = T(det(pfx + what + ".z", (n, B))) > 1.0
    x[:, :, 0][m] = 0.0
    return x


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("tag,pfx,bi,d,H,L,Tn,S,mask", CASES, ids=[c[0] for c in CASES])
def test_f16_standalone(prec, tag, pfx, bi, d, H, L, Tn, S, mask):
    g = load("f16_attn_maps")
    enc = TransformerEncoder(d, H, L, attn_mask=mask, biprojection=bi)
    enc.precision = prec
    with torch.no_grad():
        for k, p in enc.named_parameters():
            p.copy_(T(det_param(pfx + k, p.shape)))
    enc = enc.cuda().train()
    x = _inputs(pfx, "x", Tn, d)
    x[-2:] = 0.0
    with pytest.raises(RuntimeError, match="forward"):
        enc.attention_maps()
    if S:
        kv = _inputs(pfx, "kv", S, d).cuda()
        enc(x.cuda(), kv, kv)
    else:
        enc(x.cuda())
    maps = enc.attention_maps()
    blocks = (("self",) if bi or not S else ()) + (("cross",) if S else ())
    assert len(maps) == L
    worst = [0.0, 0.0]
    for i, m in enumerate(maps):
        assert tuple(m) == blocks
        for blk in blocks:
            ref = g[f"{tag}.L{i}.{blk}"]
            w = m[blk].weights
            assert m[blk].query_steps is None and w.dtype == torch.float32 and w.is_contiguous() and not w.requires_grad
            Sk = ref.shape[-1]
            assert (w[:, T(_hidden(Tn, Sk, mask)).cuda()] == 0).all(), f"L{i}.{blk}: masked entries must be exactly 0"
            e, r = _errors(w, ref)
            worst = [max(worst[0], e), max(worst[1], r)]
    _note(prec, tag, *worst)
    print(f"{prec} {tag}: max-abs {worst[0]:.3e} rel-L2 {worst[1]:.3e}")
    if prec == "f32":
        assert worst[0] <= F32_LIMIT, f"max err {worst[0]:.3e} > {F32_LIMIT:.1e}"
    else:
        lim = MEASURED[f"{prec}.{tag}"]
        assert worst[0] <= 2 * lim["max_abs"] and worst[1] <= 2 * lim["rel_l2"], \
            f"max-abs {worst[0]:.3e} (limit {2 * lim['max_abs']:.2e}), rel-L2 {worst[1]:.3e} (limit {2 * lim['rel_l2']:.2e})"


def args_for(model, **kw):
    a = dict(model=model, orig_d_l=768, orig_d_v=35, orig_d_a=74, orig_d_p=4096, hidden_sz=300, vonly=True, lonly=True,
             aonly=True, num_heads=12, layers=8, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.,
             res_dropout=0., out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6,
             bert_model="unused", text_features=True)
    a.update(kw)
    return SimpleNamespace(**a)


def _close_norm(w, ref, det_w, what):
    """F15's norm / sum check: |n - n_ref| and |s - s_ref| / sqrt(numel) within the limit times n_ref."""
    t = w.detach().double().cpu()
    if det_w is not None:
        t = t * det_w
    n, s = float(t.norm()), float(t.sum())
    err = max(abs(n - ref[0]), abs(s - ref[1]) / np.sqrt(t.numel())) / max(ref[0], 1e-6)
    assert err <= F32_LIMIT, f"norm / sum of {what}: {n:.6e} / {s:.6e} vs {ref[0]:.6e} / {ref[1]:.6e} (err {err:.2e})"


@pytest.mark.skipif(os.environ.get("BPMULT_GRAPH", "1") == "0", reason="graph replay switched off by BPMULT_GRAPH=0")
@pytest.mark.parametrize("prune", [pytest.param(False, id="dense"), pytest.param(True, id="pruned")])
def test_f16_model(prune):
    """mmtrvat at F7's configuration, f32: after the first (eager) call and after the fourth (a graph replay)."""
    from bpmult_amd.models.bpmult import LEVEL2
    g = load("f16_attn_maps")
    rows = g["m.query_rows"]
    model = get_model(args_for("mmtrvat", hidden_sz=24, num_heads=4, layers=2, orig_d_l=32))
    model.set_prune_unused_rows(prune)
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(T(det_param("f7." + k, p.shape)))
    model.precision = "f32"
    model = model.cuda().train()
    xs = [T(det("f7.xl", (2, 50, 32))).cuda(), T(det("f7.img", (2, 500, 35))).cuda(), T(det("f7.aud", (2, 375, 74))).cuda()]
    logits_ref = load("f7_mmtrvat")["logits"]
    with pytest.raises(RuntimeError, match="forward"):
        model.attention_maps()
    for call in range(4):
        logits = model(xs[0], None, None, xs[1], xs[2])
        assert float(np.abs(logits.detach().cpu().numpy() - logits_ref).max()) <= 1e-4 * max(1.0, float(np.abs(logits_ref).max()))
        if call not in (0, 3):
            continue
        trunk = model._trunks[2]
        if call == 3:
            assert any("graph" in e for e in trunk._fg.values()), "the fourth call is a graph replay"
        maps = model.attention_maps()
        assert sorted(maps) == sorted(g["m.names"].tolist())
        for n, per_layer in maps.items():
            assert len(per_layer) == 2
            for i, m in enumerate(per_layer):
                assert tuple(m) == ("cross",)
                w, steps = m["cross"]
                ref = g[f"m.{n}.L{i}.rows"]
                if prune and n in LEVEL2:
                    assert steps == (0, 511) and w.shape == (2, 2, 512)
                    e, _ = _errors(w, ref[:, [0, 7]])
                    assert (w[:, 0, 1:] == 0).all()
                else:
                    assert steps is None and w.shape == (2, 512, 512)
                    e, _ = _errors(w[:, T(rows).cuda()], ref)
                    assert (w[:, T(_hidden(512, 512, True)).cuda()] == 0).all()
                    _close_norm(w, g[f"m.{n}.L{i}.n"], None, f"{n}.L{i}")
                    _close_norm(w, g[f"m.{n}.L{i}.wn"], T(det(f"f16m.w.{n}.L{i}", (2, 512, 512))).double(), f"{n}.L{i} * w")
                assert e <= F32_LIMIT, f"call {call} {n}.L{i}: max err {e:.3e}"
        # selection
        sel = model.attention_maps(names=["trans_a_with_v2l"], layers=[1])
        assert list(sel) == ["trans_a_with_v2l"] and len(sel["trans_a_with_v2l"]) == 1
        assert torch.equal(sel["trans_a_with_v2l"][0]["cross"].weights, maps["trans_a_with_v2l"][1]["cross"].weights)


# ---------------------------------------------------------------------------------------------------------------------
# 3. properties
# ---------------------------------------------------------------------------------------------------------------------
DROP = dict(attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.25, out_dropout=0.1)      # README rates


def _toy(model="mmtrvat", seed=3, **kw):
    torch.manual_seed(seed)
    if model == "mmtrvapt":
        a = args_for("mmtrvapt", hidden_sz=24, num_heads=4, layers=2, orig_d_l=32, orig_d_v=40, orig_d_a=96, orig_d_p=64,
                     n_classes=13, num_vectors_l=96, num_vectors_a=56, num_vectors_v=56, **kw)
    else:
        a = args_for("mmtrvat", hidden_sz=24, num_heads=4, layers=2, orig_d_l=32, num_vectors_l=80, num_vectors_a=48,
                     num_vectors_v=72, **kw)
    m = get_model(a)
    if model == "mmtrvapt":
        m.audio_enc.conv_layers[2] = torch.nn.AdaptiveAvgPool1d(56)
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m


def _toy_inputs(model="mmtrvat", seed=4):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    if model == "mmtrvapt":
        return [r(2, 40, 32), r(2, 50, 40), r(2, 96, 700), r(2, 64)]
    return [r(2, 17, 32), r(2, 48, 35), r(2, 31, 74)]


def _call(m, x, **kw):
    return m(x[0], None, None, *x[1:], **kw)


def _flat(maps):
    return [(n, i, blk, mp) for n, per in maps.items() for i, d_ in enumerate(per) for blk, mp in d_.items()]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("model", ["mmtrvat", "mmtrvapt"])
def test_training_mode_properties(prec, model):
    """README dropout rates on: rows sum to 1 (the maps are taken before dropout), masked entries are exactly 0, two
    calls return identical tensors, backward() leaves them bit-equal, another input changes them."""
    dtype = BPM_F32 if prec == "f32" else BPM_BF16
    m = _toy(model, **DROP)
    m.precision = prec
    m = m.cuda().train()
    x = _toy_inputs(model)
    logits = _call(m, x)
    a = m.attention_maps()
    b = m.attention_maps()
    trunk = m._trunks[2]
    for (n, i, blk, ma), (_, _, _, mb) in zip(_flat(a), _flat(b)):
        w = ma.weights
        assert torch.equal(w, mb.weights) and w.data_ptr() != mb.weights.data_ptr(), (n, i, blk)
        err = float((w.double().sum(-1) - 1.0).abs().max())
        assert err <= tol(dtype), f"{n}.L{i}.{blk}: row sums off by {err:.3e}"
        Sk = w.shape[-1]
        steps = ma.query_steps
        Tfull = trunk.N["l" if n.startswith("trans_l") else "v" if n.startswith("trans_v") else "a"]
        times = torch.arange(Tfull) if steps is None else torch.tensor(steps)
        assert w.shape[1] == len(times)
        hidden = ((torch.arange(Sk)[None, :] - times[:, None]) >= 1 + abs(Sk - Tfull)).cuda()
        assert (w[:, hidden] == 0).all(), (n, i, blk)
    logits.sum().backward()
    c = m.attention_maps()
    for (n, i, blk, ma), (_, _, _, mc) in zip(_flat(a), _flat(c)):
        assert torch.equal(ma.weights, mc.weights), f"{n}.L{i}.{blk}: backward() changed the map"
    _call(m, _toy_inputs(model, seed=9))
    d_ = m.attention_maps()
    assert all(not torch.equal(ma.weights, md.weights) for (_, _, _, ma), (_, _, _, md) in zip(_flat(a), _flat(d_)))
    m.eval()
    with torch.no_grad():
        _call(m, x)
        e = m.attention_maps(layers=[0])
    assert all(len(v) == 1 for v in e.values())


def test_four_modal_pruned_maps_are_rows_of_the_dense_ones():
    m1 = _toy("mmtrvapt")
    m1.precision = "f32"
    m2 = copy.deepcopy(m1)
    m1, m2 = m1.cuda().train(), m2.cuda().train()
    m1.set_prune_unused_rows(False)
    m2.set_prune_unused_rows(True)
    x = _toy_inputs("mmtrvapt")
    _call(m1, x)
    _call(m2, x)
    dense, pruned = m1.attention_maps(), m2.attention_maps()
    few = 0
    for (n, i, blk, md), (_, _, _, mp) in zip(_flat(dense), _flat(pruned)):
        assert md.query_steps is None
        ref = md.weights if mp.query_steps is None else md.weights[:, list(mp.query_steps)]
        few += mp.query_steps is not None
        assert mp.weights.shape == ref.shape, (n, i, blk)
        assert float((mp.weights - ref).abs().max()) <= F32_LIMIT, (n, i, blk)
    assert few == 6 * 2                                   # the last layer of the six level-2 encoders: self and cross


@pytest.mark.skipif(os.environ.get("BPMULT_GRAPH", "1") == "0", reason="graph replay switched off by BPMULT_GRAPH=0")
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
def test_taking_the_maps_does_not_disturb_the_step(graphs):
    """forward + attention_maps + backward against forward + backward on a copy of the model, README dropout rates on,
    four steps (with graphs: the later ones are replays).  Logits, gates, loss, the input gradients and the gradients of
    the encoder matrices are bit-equal.  The gradients that are summed by float atomics or arrive from two streams (tail,
    LayerNorm affines, biases) differ between two runs of the SAME step in the last bits, so they are held to the 1e-5
    that tests/test_model_gpu.py::test_graph_replay_equals_eager_launches holds them to."""
    m1 = _toy(**DROP)
    m1.precision = "bf16"
    m2 = copy.deepcopy(m1)
    m1, m2 = m1.cuda().train(), m2.cuda().train()
    m1.use_graphs = m2.use_graphs = graphs
    tgt = (torch.randn(2, 6, generator=torch.Generator().manual_seed(1)) > 0).float().cuda()
    x = _toy_inputs()
    for step in range(4):
        outs = []
        for m, take in ((m1, False), (m2, True)):
            for p in m.parameters():
                p.grad = None
            xs = [t.clone().requires_grad_(True) for t in x]
            logits, z = _call(m, xs, output_gate=True)
            if take:
                maps = m.attention_maps()
                assert len(maps) == 12
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt)
            loss.backward()
            outs.append((logits.detach().clone(), z.detach().clone(), loss.detach().clone(), [t.grad.clone() for t in xs],
                         {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
        a, b = outs
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), f"step {step}"
        for u, v in zip(a[3], b[3]):
            assert torch.equal(u, v), f"step {step}: input gradients differ"
        assert a[4].keys() == b[4].keys()
        for k in a[4]:
            if "gmu." in k or k.startswith(("proj1", "proj2", "out_layer")) or "layer_norm" in k or "bias" in k:
                assert float((a[4][k] - b[4][k]).abs().max()) <= 1e-5 * max(1.0, float(a[4][k].abs().max())), (step, k)
            else:
                assert torch.equal(a[4][k], b[4][k]), f"step {step}: gradient of {k} differs"
    if graphs:
        assert any("graph" in e for e in m2._trunks[2]._fg.values())


def test_encoder_maps_survive_backward_and_follow_the_last_call_form():
    enc = TransformerEncoder(24, 4, 2, attn_dropout=0.1, res_dropout=0.1, attn_mask=True, biprojection=True).cuda().train()
    x = rnd(9, 2, 24, seed=1).cuda().requires_grad_(True)
    kv = rnd(12, 2, 24, seed=2).cuda()
    y = enc(x, kv, kv)
    a = enc.attention_maps()
    assert [tuple(m) for m in a] == [("self", "cross")] * 2 and a[0]["cross"].weights.shape == (2, 9, 12)
    y.sum().backward()
    c = enc.attention_maps()
    assert all(torch.equal(a[i][k].weights, c[i][k].weights) for i in range(2) for k in ("self", "cross"))
    enc(x)                                             # the other call form: its own plan
    s = enc.attention_maps(layers=[1])
    assert [tuple(m) for m in s] == [("self",)] and s[0]["self"].weights.shape == (2, 9, 9)
    enc = enc.cpu().cuda()                             # buffers dropped
    with pytest.raises(RuntimeError, match="forward"):
        enc.attention_maps()
