"""bpmult_amd.models.MultiheadAttention.forward on the MI355X against the reference's own MultiheadAttention
(tests/golden/mha.npz, written by tests/golden/make_golden_mha.py on the CPU in eval mode; cases in tests/mha_cases.py):
attn, the head-averaged weights, and the gradients of the inputs and of every parameter under a fixed upstream gradient.

f32 mode: max error <= 2e-4 * max(1, |ref|max), the limit tests/test_encoder_gpu.py holds F5 to in f32.
bf16 mode: relative L2 error of the tensor per kind of tensor, <= 2x the errors measured against the fixture on the MI355X
(profiles/mha_errors.json, written by this file's `_note` through BPMULT_ERROR_LOG), and never looser than
tests/test_encoder_gpu.py's bf16 limit for the same kind (y 1e-2, input gradients 1e-1, weights / biases 1.4e-1); the max
error is held to 4x the limit, as there.
Measured rel-L2 maxima over the four cases: attn 5.0e-3, weights 1.3e-3, input gradients 6.2e-3, weight gradients 4.9e-3,
bias gradients 3.6e-3.  The weights have no counterpart in test_encoder_gpu.py: 2x the measured value."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detgen import det, det_param  # noqa: E402
from mha_cases import CASES, make_mask  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import ops  # noqa: E402
from bpmult_amd.models import MultiheadAttention  # noqa: E402
from bpmult_amd.ops import BPM_F32  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = dict(np.load(os.path.join(ROOT, "tests", "golden", "mha.npz")))
T = torch.from_numpy
F32_LIMIT = 2e-4
# bf16, rel-L2 per kind: min(2 x measured, the limit of tests/test_encoder_gpu.py for the kind)
BF16_LIMIT = {"attn": 1.0e-2, "weights": 2.6e-3, "gx": 1.2e-2, "weight": 9.9e-3, "bias": 7.2e-3}
ENCODER_BF16_LIMIT = {"attn": 1e-2, "gx": 1e-1, "weight": 1.4e-1, "bias": 1.4e-1}
assert all(BF16_LIMIT[k] <= v for k, v in ENCODER_BF16_LIMIT.items())

_MEASURED = {}
# where the measured errors go (the JSON of profiles/mha_errors.json): set BPMULT_ERROR_LOG to a file path to record
# them; unset, nothing is written
_LOG = os.environ.get("BPMULT_ERROR_LOG")


def kind_of(name):
    return name if name in ("attn", "weights") else "gx" if name in ("gq", "gk", "gv") else "bias" if name.endswith("bias") else "weight"


def _note(prec, tag, name, rel, err):
    """Largest error per (precision, case, tensor kind), written to the file BPMULT_ERROR_LOG names (the JSON committed as
    profiles/mha_errors.json): the bf16 limits above are 2x the rel_l2 maxima over the cases."""
    key = f"{prec}.{tag}.{kind_of(name)}"
    m = _MEASURED.setdefault(key, {"rel_l2": 0.0, "max_abs": 0.0})
    m["rel_l2"], m["max_abs"] = max(m["rel_l2"], rel), max(m["max_abs"], err)
    if not _LOG:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(_LOG)), exist_ok=True)
        json.dump(_MEASURED, open(_LOG, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def build(case, prec, dropout=0.0):
    tag, form, Tn, S, B, d, H, kind, bias = case
    pfx = tag + "."
    m = MultiheadAttention(d, H, attn_dropout=dropout, bias=bias)
    m.precision = prec
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(T(det_param(pfx + k, p.shape)))
    m = m.cuda()
    q = T(det(pfx + "q", (Tn, B, d))).cuda().requires_grad_(True)
    if form == "qkv":
        k = v = q
    elif form == "kv":
        k = v = T(det(pfx + "k", (S, B, d))).cuda().requires_grad_(True)
    else:
        k, v = (T(det(pfx + n, (S, B, d))).cuda().requires_grad_(True) for n in ("k", "v"))
    mask = make_mask(kind, Tn, S, pfx)
    mask = None if mask is None else T(mask).cuda()
    w = T(det(pfx + "w", (Tn, B, d))).cuda()
    return m, q, k, v, mask, w


def step(m, q, k, v, mask, w, need_weights=True):
    """One forward + backward from clean gradients -> {name: tensor}."""
    for t in [q, k, v] + list(m.parameters()):
        t.grad = None
    y, wt = m(q, k, v, attn_mask=mask, need_weights=need_weights)
    (y * w).sum().backward()
    torch.cuda.synchronize()
    out = {"attn": y.detach(), "weights": wt, "gq": q.grad.clone()}      # copies: a later backward adds into .grad in place
    if k is not q:
        out["gk"] = k.grad.clone()
    if v is not k:
        out["gv"] = v.grad.clone()
    for n, p in m.named_parameters():
        out["g." + n] = p.grad.clone()
    return out


def same(a, b, n):
    """Bit-equal -- except the bias gradients, column sums by float atomics: equal up to the order of summation."""
    if n.endswith("bias"):
        return torch.allclose(a, b, rtol=1e-5, atol=1e-5 * float(b.abs().max()))
    return torch.equal(a, b)


_RUNS = {}


def run(tag, prec):
    if (tag, prec) not in _RUNS:
        case = next(c for c in CASES if c[0] == tag)
        m, q, k, v, mask, w = build(case, prec)
        m.eval()
        _RUNS[(tag, prec)] = (step(m, q, k, v, mask, w), m)
    return _RUNS[(tag, prec)]


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_module_matches_the_reference(tag, prec):
    got, _ = run(tag, prec)
    names = sorted(k[len(tag) + 1:] for k in G if k.startswith(tag + ".") and not k.endswith((".idx", ".n")))
    assert sorted(got) == names, (sorted(got), names)
    wt = got["weights"]
    assert wt is not None and not wt.requires_grad and wt.dtype == torch.float32
    for name in names:
        key = f"{tag}.{name}"
        a = got[name].detach().float().cpu().numpy()
        ref, idx, (rn, _) = G[key], G.get(key + ".idx"), G[key + ".n"]
        assert np.isfinite(a).all(), key
        whole, n_whole = float(np.linalg.norm(a.astype(np.float64).ravel())), a.size
        if idx is not None:
            a = np.take(a, idx, axis=1 if name == "weights" else 0)
        assert a.shape == ref.shape, (key, a.shape, ref.shape)
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(a - ref).max())
        rel = float(np.linalg.norm((a - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-6))
        _note(prec, tag, name, rel, err)
        print(f"{prec} {key}: max err {err:.3e} (scale {scale:.3g}), rel-L2 {rel:.3e}")
        if prec == "f32":
            assert err <= F32_LIMIT * scale, f"{key}: max err {err:.3e} > {F32_LIMIT * scale:.3e}"
            lim = F32_LIMIT
        else:
            lim = BF16_LIMIT[kind_of(name)]
            assert rel <= lim and err <= 4 * lim * scale, f"{key}: rel-L2 {rel:.3e} (limit {lim:.1e}), max err {err:.3e} (scale {scale:.3g})"
        # the whole tensor, where only every fourth slice is stored: | ||a|| - ||ref|| | <= ||a - ref||, which is at most
        # sqrt(N) * (the max-error limit) in f32 and (the rel-L2 limit) * ||ref|| in bf16
        bound = np.sqrt(n_whole) * F32_LIMIT * scale if prec == "f32" else lim * max(rn, 1e-6)
        assert abs(whole - rn) <= bound, f"{key}: norm {whole:.6g} vs {rn:.6g} (bound {bound:.3g})"
    if tag in ("m1", "m2"):          # hidden pairs are exact zeros in the weights, every row sums to 1
        case = next(c for c in CASES if c[0] == tag)
        hidden = np.isinf(make_mask(case[7], case[2], case[3], tag + "."))
        wn = wt.cpu().numpy()
        assert (wn[:, hidden] == 0).all()
        assert float(np.abs(wn.astype(np.float64).sum(-1) - 1).max()) <= (2e-5 if prec == "f32" else 1.5e-2)


def test_future_mask_tensor_agrees_with_the_mask_off_rule():
    """M1: the -inf triangular tensor through the *_amask kernels against the same attention expressed through the
    mask_off rule (the unmasked entries on the module's own Q / K / V / dO buffers), within the f32 kernel limits of
    tests/test_attn_amask_gpu.py (forward, lse 3e-5; dQ, dK, dV 1e-4, relative to max(1, |ref|max))."""
    _, m = run("m1", "f32")
    ex = m._exec
    (pl,) = ex.plans.values()
    Tn, S, B, H, dh, dhp, ld = pl.T, pl.S, pl.B, ex.H, ex.dh, ex.dhp, ex.ld
    assert pl.mask is not None and ex.dtype == BPM_F32
    O, lse, delta = torch.zeros_like(pl.o), torch.zeros_like(pl.lse), torch.zeros_like(pl.delta)
    dq, dk, dv = torch.zeros_like(pl.dq), torch.zeros_like(pl.dk), torch.zeros_like(pl.dv)
    p = ops.attn_problem(pl.q, pl.k, pl.v, O, ld, lse, B, H, Tn, S, dh, dhp, 1 + abs(S - Tn), dO=pl.dao, delta=delta, dQ=dq, lddq=ld,
                         dK=dk, lddk=ld, dV=dv, lddv=ld, dq_scale=ex.scale)
    ops.attn_fwd(BPM_F32, [p])
    ops.attn_bwd_dq(BPM_F32, [p])
    ops.attn_bwd_dkv(BPM_F32, [p])
    torch.cuda.synchronize()
    for a, b, t, nm in ((pl.o, O, 3e-5, "O"), (pl.lse, lse, 3e-5, "lse"), (pl.dq, dq, 1e-4, "dQ"), (pl.dk, dk, 1e-4, "dK"), (pl.dv, dv, 1e-4, "dV")):
        assert torch.isfinite(a).all(), nm
        err, scale = float((a - b).abs().max()), max(1.0, float(b.abs().max()))
        assert float(b.abs().max()) > 0 and err <= t * scale, f"{nm}: {err:.3e} > {t * scale:.3e}"


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_need_weights_false_launches_nothing_for_them(prec, monkeypatch):
    m, q, k, v, mask, w = build(CASES[1], prec)
    m.eval()
    a = step(m, q, k, v, mask, w)
    calls = []
    for fn in ("attn_maps", "attn_maps_amask"):
        monkeypatch.setattr(ops, fn, lambda *a_, _fn=fn, **k_: calls.append(_fn))
    b = step(m, q, k, v, mask, w, need_weights=False)
    assert b["weights"] is None and a["weights"] is not None and not calls
    for n in a:
        if n != "weights":
            assert same(a[n], b[n], n), n


def test_dropout_is_reproducible_from_the_torch_seed():
    outs = []
    for _ in range(2):
        torch.manual_seed(1234)
        m, q, k, v, mask, w = build(CASES[1], "bf16", dropout=0.1)
        m.train()
        outs.append((step(m, q, k, v, mask, w), step(m, q, k, v, mask, w)))
    (a1, a2), (b1, b2) = outs
    for n in a1:
        assert same(a1[n], b1[n], n) and same(a2[n], b2[n], n), n
    assert not torch.equal(a1["attn"], a2["attn"]), "the next call must draw another dropout mask"
    assert torch.equal(a1["weights"], a2["weights"]), "the returned weights are taken before dropout"
    m.eval()
    e = step(m, q, k, v, mask, w)
    assert not torch.equal(e["attn"], a1["attn"])


def test_parameters_stay_torch_owned():
    m, q, k, v, mask, w = build(CASES[3], "f32")
    m.eval()
    a = step(m, q, k, v, mask, w)
    # a second backward accumulates into .grad
    y, _ = m(q, k, v, attn_mask=mask)
    (y * w).sum().backward()
    for n, p in m.named_parameters():
        assert torch.allclose(p.grad, 2 * a["g." + n], rtol=1e-5, atol=1e-5 * float(a["g." + n].abs().max())), n
    assert torch.allclose(q.grad, 2 * a["gq"], rtol=1e-5, atol=1e-7)
    # editing a weight in place moves its version counter: the shadow is re-packed, the next output changes
    with torch.no_grad():
        m.out_proj.weight.mul_(2.0)
    b = step(m, q, k, v, mask, w)
    assert not torch.equal(a["attn"], b["attn"])
    bias = m.out_proj.bias.detach()
    assert torch.allclose(b["attn"] - bias, 2 * (a["attn"] - bias), rtol=1e-4, atol=1e-5)
    # .to() drops plans and shadows
    assert m._exec is not None and m._exec.plans
    m.cuda()
    assert m._exec is None
    assert torch.equal(step(m, q, k, v, mask, w)["attn"], b["attn"])


def test_a_mask_modified_in_place_is_read_again():
    m, q, k, v, mask, w = build(CASES[3], "f32")
    m.eval()
    a = step(m, q, k, v, mask, w)
    cached = m._exec._mask
    assert torch.equal(step(m, q, k, v, mask, w)["attn"], a["attn"]) and m._exec._mask is cached      # same tensor, same version: kept
    mask[:, 3] = float("-inf")
    b = step(m, q, k, v, mask, w)
    assert m._exec._mask is not cached and not torch.equal(a["attn"], b["attn"])
    c = step(m, q, k, v, mask.clone(), w)
    for n in b:
        assert same(b[n], c[n], n), n
    assert float(b["weights"][:, :, 3].abs().max()) == 0.0
    with pytest.raises(ValueError, match="no gradient"):
        m(q, k, v, attn_mask=mask.clone().requires_grad_(True))
    m.precision = "bf16x3"
    with pytest.raises(ValueError, match="bf16x3"):
        m(q, k, v, attn_mask=mask)
