"""The self-attention stack TransformerEncoder.forward(x) (engine GroupCfg.self_only) on the MI355X, against the REAL
reference's forward(x): F5 case `s` and every case of F15 (tests/golden/make_golden_self_attn.py), in f32, bf16 and
bf16x3, output, input gradient and every parameter gradient.  Limits:
  f32     2e-4 of the tensor's max (as test_encoder_gpu.py; gradient norms / sums: 2e-4 relative)
  bf16x3  1e-3 of the tensor's max (as the model tests)
  bf16    relative L2 error per case and kind of tensor, <= 2x the error measured on the MI355X
          (profiles/r05_self_encoder_errors.json, see BF16_MEASURED)
Then: eval / no_grad forward, backward regenerating forward's dropout masks (central differences with every dropout on),
one module called both ways, and a lock-step group of three self-only encoders."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detgen import det, det_param  # noqa: E402

import bpmult_amd  # noqa: E402
from bpmult_amd import engine  # noqa: E402
from bpmult_amd._lib import BPM_F32  # noqa: E402
from bpmult_amd.models.encoder import TransformerEncoder  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
B = 2

# (fixture, case, biprojection, d, heads, layers, T, attn_mask)
CASES = [("f5_encoder", "s", False, 24, 4, 2, 6, True),
         ("f15_self_encoder", "sb", True, 24, 4, 2, 7, True), ("f15_self_encoder", "sn", False, 24, 4, 2, 9, False),
         ("f15_self_encoder", "s25", False, 50, 2, 2, 70, True), ("f15_self_encoder", "s128", False, 256, 2, 2, 130, True),
         ("f15_self_encoder", "s256", True, 512, 2, 1, 40, True)]
TOL = {"f32": 2e-4, "bf16x3": 1e-3}
# bf16: the largest relative L2 error per case and kind of tensor measured on the first MI355X run (rounded up to two
# digits; profiles/r05_self_encoder_errors.json, "bf16.*"); the limit is 2x.  "norm": the norm / sum check of the tensors
# stored as norm and sum only.  sb (biprojection, d=24) is the noisiest: its zero-padded rows reach the input gradient
# through a LayerNorm of a near-constant row.
BF16_MEASURED = {
    "s": {"y": 0.0035, "gx": 0.028, "weight": 0.052, "bias": 0.052, "layer_norm": 0.067},
    "sb": {"y": 0.0032, "gx": 0.16, "weight": 0.17, "bias": 0.17, "layer_norm": 0.22, "norm": 0.065},
    "sn": {"y": 0.0024, "gx": 0.0059, "weight": 0.013, "bias": 0.013, "layer_norm": 0.028, "norm": 0.0047},
    "s25": {"y": 0.00085, "gx": 0.0082, "weight": 0.0068, "bias": 0.026, "layer_norm": 0.024, "norm": 0.0048},
    "s128": {"y": 0.0012, "gx": 0.06, "bias": 0.072, "layer_norm": 0.063, "norm": 0.014},
    "s256": {"y": 0.0011, "gx": 0.055, "bias": 0.052, "layer_norm": 0.053, "norm": 0.0041},
}


def bf16_limit(tag, what):
    return 2.0 * BF16_MEASURED[tag][kind(what)]


_FIX = {}
_MEASURED = {}
# where the measured errors go (the JSON of profiles/r05_self_encoder_errors.json): set BPMULT_ERROR_LOG to a file path to
# record them; unset, nothing is written
_LOG = os.environ.get("BPMULT_ERROR_LOG")


def load(name):
    if name not in _FIX:
        _FIX[name] = dict(np.load(os.path.join(G, name + ".npz")))
    return _FIX[name]


def kind(what):
    return what if what in ("y", "gx", "norm") else "layer_norm" if "layer_norm" in what else "bias" if "bias" in what else "weight"


def _note(prec, tag, what, err):
    """Largest error per (precision, case, kind): relative L2 in bf16 mode, error / max(1, |ref|max) otherwise."""
    key = f"{prec}.{tag}.{kind(what)}"
    _MEASURED[key] = max(_MEASURED.get(key, 0.0), err)
    if not _LOG:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(_LOG)), exist_ok=True)
        with open(_LOG, "w") as f:
            json.dump(_MEASURED, f, indent=1, sort_keys=True)
    except OSError:
        pass


def close(a, b, prec, what, tag, bad):
    """Appends a failure to `bad` (every tensor of a case is measured before the test fails)."""
    a = a.detach().double().cpu().numpy()
    b = b.astype(np.float64)
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what
    if prec == "bf16":
        rel = float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-6))
        _note(prec, tag, what, rel)
        if rel > bf16_limit(tag, what):
            bad.append(f"{what}: rel-L2 {rel:.3e} > {bf16_limit(tag, what):.2e}")
    else:
        err = float(np.abs(a - b).max()) / max(1.0, float(np.abs(b).max()))
        _note(prec, tag, what, err)
        if err > TOL[prec]:
            bad.append(f"{what}: max err {err:.3e} (of max(1, |ref|)) > {TOL[prec]:.1e}")


def close_norm(t, ref, prec, what, tag, bad):
    """Norm and sum of a whole tensor against the reference's (float64): |n - n_ref| and |s - s_ref| within the limit times
    n_ref (the sum bound scaled by sqrt(numel), |sum(e)| <= sqrt(n) |e|)."""
    t = t.detach().double().cpu()
    n, s = float(t.norm()), float(t.sum())
    lim = bf16_limit(tag, "norm") if prec == "bf16" else TOL[prec]
    err = max(abs(n - ref[0]), abs(s - ref[1]) / np.sqrt(t.numel())) / max(ref[0], 1e-6)
    _note(prec, tag, "norm", err)
    if err > lim:
        bad.append(f"norm / sum of {what}: {n:.6e} / {s:.6e} vs {ref[0]:.6e} / {ref[1]:.6e} (err {err:.2e} > {lim:.1e})")


def make(bi, d, H, L, mask, prec, pfx, **kw):
    enc = TransformerEncoder(d, H, L, attn_mask=mask, biprojection=bi, **kw)
    enc.precision = prec
    with torch.no_grad():
        for k, p in enc.named_parameters():
            p.copy_(T(det_param(pfx + k, p.shape)))
    return enc.cuda().train()


def inputs(pfx, Tn, d):
    x = T(det(pfx + "x", (Tn, B, d)))
    m = T(det(pfx + "x.z", (Tn, B))) > 1.0
    x[:, :, 0][m] = 0.0
    x[-2:] = 0.0
    return x


def _pfx(fix, tag):
    return ("f5" if fix == "f5_encoder" else "f15") + tag + "."


@pytest.mark.parametrize("prec", ["f32", "bf16", "bf16x3"])
@pytest.mark.parametrize("fix,tag,bi,d,H,L,Tn,mask", CASES, ids=[c[1] for c in CASES])
def test_self_encoder_against_reference(prec, fix, tag, bi, d, H, L, Tn, mask):
    g = load(fix)
    pfx = _pfx(fix, tag)
    enc = make(bi, d, H, L, mask, prec, pfx)
    x = inputs(pfx, Tn, d).cuda().requires_grad_(True)
    y = enc(x)
    assert y.shape == (Tn, B, d)
    (y * T(det(pfx + "w", tuple(y.shape))).cuda()).sum().backward()
    rows = torch.from_numpy(g.get(f"{tag}.rows", np.arange(Tn))).cuda()
    bad = []
    close(y[rows], g[f"{tag}.y"], prec, "y", tag, bad)
    close(x.grad[rows], g[f"{tag}.gx"], prec, "gx", tag, bad)
    if f"{tag}.yn" in g:
        close_norm(y, g[f"{tag}.yn"], prec, "y", tag, bad)
        close_norm(x.grad, g[f"{tag}.gxn"], prec, "gx", tag, bad)
    nograd = set(g[f"{tag}.nograd"].tolist()) if f"{tag}.nograd" in g else set()
    if bi:
        assert nograd == {f"layers.{i}.layer_norms.1.{w}" for i in range(L) for w in ("weight", "bias")}
    for k, p in enc.named_parameters():
        if k in nograd:                      # unused by the reference's call: None or all-zero (as transfm_* in the models)
            assert p.grad is None or not bool(p.grad.any()), k
            continue
        assert p.grad is not None, k
        if f"{tag}.g.{k}" in g:
            close(p.grad, g[f"{tag}.g.{k}"], prec, k, tag, bad)
        if f"{tag}.gn.{k}" in g:
            close_norm(p.grad, g[f"{tag}.gn.{k}"], prec, k, tag, bad)
        else:
            assert f"{tag}.g.{k}" in g, k
    assert not bad, bad


@pytest.mark.parametrize("bi", [False, True])
def test_eval_and_no_grad_equal_train_without_dropout(bi):
    d, H, L, Tn = 48, 4, 2, 21
    enc = make(bi, d, H, L, True, "f32", "self_eval.")
    x = inputs("self_eval.", Tn, d).cuda()
    y_train = enc(x.clone().requires_grad_(True)).detach()
    with torch.no_grad():
        y_ng = enc(x)
    enc.eval()
    y_eval = enc(x)
    for y in (y_ng, y_eval.detach()):
        assert float((y - y_train).abs().max()) <= 1e-6 * max(1.0, float(y_train.abs().max()))


# Central differences in f32 with every dropout on (seed step held fixed: the same masks in every pass), along the
# computed gradient g itself (input and every parameter, scaled to max |v| = 1): the directional derivative is |g|^2 and
# the central difference <g_true, g>, so a gradient error dg shows as <dg, g_true> + |dg|^2 -- never cancelled by a random
# direction.  The input has no zero-padded rows: the channel-0 padding rule is a step function of the input, and the
# LayerNorm of an all-zero row has rstd = 1/sqrt(eps).
# One run on the MI355X (profiles/r05_self_encoder_errors.json, "f32.fd_*"), relative error at steps 3e-4 / 1e-3 / 3e-3 /
# 1e-2: 6.0e-6 / 4.7e-5 / 2.5e-4 / 7.0e-4 (plain layers), 2.9e-5 / 3.7e-6 / 2.0e-5 / 2.2e-4 (biprojection).
# EPS = 1e-3, FD_TOL = 1e-3 (20x the larger of the two).
EPS, FD_TOL = 1e-3, 1e-3


@pytest.mark.parametrize("bi", [False, True])
def test_dropout_masks_regenerated_in_backward(bi):
    d, H, L, Tn = 32, 4, 2, 11
    pfx = "self_fd."
    enc = make(bi, d, H, L, True, "f32", pfx, attn_dropout=0.2, relu_dropout=0.2, res_dropout=0.2, embed_dropout=0.2)
    x0 = T(det(pfx + "x", (Tn, B, d))).cuda()
    w = T(det(pfx + "w", (Tn, B, d))).cuda()
    params = [p for _, p in enc.named_parameters()]

    def f(x):
        enc._step = 1000                       # the same seed in every pass
        return enc(x)

    x = x0.clone().requires_grad_(True)
    y = f(x)
    enc.eval()
    assert float((enc(x0).detach() - y.detach()).abs().max()) > 1e-2, "dropout must be active in train mode"
    enc.train()
    assert torch.equal(f(x0).detach(), y.detach()), "a fixed seed step must draw the same masks"
    (y * w).sum().backward()
    gs = [x.grad.detach().clone()] + [p.grad.detach().clone() for p in params]
    gmax = max(float(g.abs().max()) for g in gs)
    vx, vp = gs[0] / gmax, [g / gmax for g in gs[1:]]
    dd = sum(float((g * g).sum()) for g in gs) / gmax

    def loss_at(h):
        with torch.no_grad():
            for p, v in zip(params, vp):
                p.add_(h * v)
            out = float((f(x0 + h * vx) * w).double().sum())
            for p, v in zip(params, vp):
                p.sub_(h * v)
        return out

    for eps in (1e-2, 3e-3, 3e-4, EPS):          # (the others only for the record)
        fd = (loss_at(eps) - loss_at(-eps)) / (2 * eps)
        rel = abs(fd - dd) / dd
        _note("f32", f"fd_bi{int(bi)}_eps{eps:g}", "y", rel)
    assert rel <= FD_TOL, f"directional derivative {dd:.6e} vs central difference {fd:.6e} (rel {rel:.2e})"


@pytest.mark.parametrize("bi", [False, True])
def test_one_module_called_both_ways(bi):
    d, H, L, Tn, S = 24, 4, 2, 9, 6
    pfx = "self_both."
    both = make(bi, d, H, L, True, "f32", pfx)
    alone_s, alone_x = (make(bi, d, H, L, True, "f32", pfx) for _ in range(2))
    x0, kv0 = inputs(pfx, Tn, d).cuda(), inputs(pfx + "kv", S, d).cuda()

    def run(m, cross):
        for p in m.parameters():
            p.grad = None
        x, kv = x0.clone().requires_grad_(True), kv0.clone().requires_grad_(True)
        y = m(x, kv, kv) if cross else m(x)
        (y * T(det(pfx + "w" + str(int(cross)), tuple(y.shape))).cuda()).sum().backward()
        return [y.detach(), x.grad] + ([kv.grad] if cross else []) + [p.grad.clone() for p in m.parameters()]

    ref_s, ref_x = run(alone_s, False), run(alone_x, True)
    for cross, ref in ((False, ref_s), (True, ref_x), (False, ref_s)):
        got = run(both, cross)
        assert len(got) == len(ref)
        for a, b in zip(got, ref):
            assert float((a - b).abs().max()) <= 1e-6 * max(1.0, float(b.abs().max()))
    assert len(both._plans) == 2


def test_lockstep_group_of_three():
    """Three self-only encoders (different lengths) in one EncoderGroupPlan against three single-encoder runs (f32)."""
    d, H, L = 48, 4, 2
    lens = (5, 17, 9)
    pf = [f"self_grp{j}." for j in range(3)]
    mods = [TransformerEncoder(d, H, L, attn_mask=True).cuda() for _ in range(3)]
    for m, p in zip(mods, pf):
        with torch.no_grad():
            for k, q in m.named_parameters():
                q.copy_(T(det_param(p + k, q.shape)))
    st = engine.ParamStore([(f"e{j}.{k}", q) for j, m in enumerate(mods) for k, q in m.named_parameters()], BPM_F32)
    for j in range(3):
        engine.register_encoder_shadows(st, f"e{j}.", d, L)
    st.finalize_shadows()
    cfg = engine.GroupCfg(d, H, L, 0.0, 0.0, 0.0, True, False, self_only=True)
    plan = engine.EncoderGroupPlan(st, cfg, [engine.EncoderDesc(f"e{j}.", j, n, n, 0.0) for j, n in enumerate(lens)], B)
    xs = [inputs(p, n, d).cuda() for p, n in zip(pf, lens)]
    ws = [T(det(p + "w", (n, B, d))).cuda() for p, n in zip(pf, lens)]
    st.refresh_shadows()
    ys = [y.clone() for y in plan.forward(xs, None, None, seed=7, training=True)]
    st.begin_backward()
    gxs, gk, gv = plan.backward(ws)
    assert gk == [None] * 3 and gv == [None] * 3
    gxs = [g.clone() for g in gxs]
    torch.cuda.synchronize()
    for j, (p, n) in enumerate(zip(pf, lens)):
        single = make(False, d, H, L, True, "f32", p)
        x = xs[j].clone().requires_grad_(True)
        y = single(x)
        (y * ws[j]).sum().backward()
        for a, b, what in [(ys[j], y.detach(), "y"), (gxs[j], x.grad, "gx")] + \
                          [(st.g(f"e{j}.{k}"), q.grad, k) for k, q in single.named_parameters()]:
            err = float((a - b).abs().max()) / max(1.0, float(b.abs().max()))
            assert err <= 2e-4, (j, what, err)
