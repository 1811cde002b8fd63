"""MultiheadAttention.forward(..., key_padding_mask=) on the MI355X, alone and beside attn_mask / attn_bias.

k1 - k3 against the reference's own sample-by-sample run (tests/golden/mha_kpm.npz, cases in tests/mha_kpm_cases.py); k4
(an [H, T, S] bias, which the reference cannot run) against the fp64 restatement of that file (tests/test_mha_kpm_cpu.py
holds it to the fixture on k1 - k3).  eval mode.

f32: max error <= 2e-4 * max(1, |ref|max) for every tensor (tests/test_mha_module_gpu.py's F32_LIMIT).
bf16: relative L2 per kind of tensor <= KPM_BF16_LIMIT = 2 x the maximum measured on the MI355X over the four cases
(profiles/mha_kpm_errors.json, written through BPMULT_ERROR_LOG; the factor 2 is the project's margin for rounding drift
between toolchains), never looser than that file's ENCODER_BF16_LIMIT (1.4e-1 for g.bias); the max error is held to 4 x the
limit.  Measured maxima (rel-L2, bf16): attn 4.12e-3 (k3), weights 1.06e-3 (k4), input gradients 6.91e-3 (k3 gq), weight
gradients 4.66e-3, projection-bias gradients 3.52e-3 (k3), g.bias 5.47e-3 (k3) -- MEASURED_BF16 below; f32: at most 1.2e-6
of the scale on every tensor.

Where two runs are compared for bit-equality (the same dropout seed; no padding mask against an all-False one), every tensor is
compared with torch.equal except g.in_proj_bias and g.out_proj.bias: those are column sums by float atomics in the GEMM and
cast launches, not results of the attention kernels, and are held to rtol 1e-5 as tests/test_mha_bias_module_gpu.py does."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from mha_kpm_cases import CASES, REFERENCE_RUNS, attn_mask, case, inputs, learned_bias, padding, restate, visible  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import ops  # noqa: E402
from bpmult_amd.models import MultiheadAttention  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = dict(np.load(os.path.join(ROOT, "tests", "golden", "mha_kpm.npz")))
T = torch.from_numpy
F32_LIMIT = 2e-4
# rel-L2 maxima over k1 - k4 on the MI355X, bf16 (profiles/mha_kpm_errors.json)
MEASURED_BF16 = {"attn": 4.12e-3, "weights": 1.06e-3, "gx": 6.91e-3, "weight": 4.66e-3, "bias": 3.52e-3, "g.bias": 5.47e-3}
CEILING = {"attn": 1e-2, "gx": 1e-1, "weight": 1.4e-1, "bias": 1.4e-1, "g.bias": 1.4e-1}      # ENCODER_BF16_LIMIT; g.bias: its `bias`
KPM_BF16_LIMIT = {k: 2 * v for k, v in MEASURED_BF16.items() if v is not None}
assert all(KPM_BF16_LIMIT[k] <= v for k, v in CEILING.items() if k in KPM_BF16_LIMIT)

_MEASURED = {}
_LOG = os.environ.get("BPMULT_ERROR_LOG")


def kind_of(name):
    if name == "g.bias":
        return "g.bias"
    return name if name in ("attn", "weights") else "gx" if name in ("gq", "gk", "gv") else "bias" if name.endswith("bias") else "weight"


def _note(prec, tag, name, rel, err):
    m = _MEASURED.setdefault(f"{prec}.{tag}.{kind_of(name)}", {"rel_l2": 0.0, "max_abs": 0.0})
    m["rel_l2"], m["max_abs"] = max(m["rel_l2"], rel), max(m["max_abs"], err)
    if not _LOG:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(_LOG)), exist_ok=True)
        json.dump(_MEASURED, open(_LOG, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def build(c, prec, dropout=0.0, train=False):
    tag, form, Tn, S, B, d, H = c[:7]
    x = inputs(c)
    m = MultiheadAttention(d, H, attn_dropout=dropout, bias=c[9])
    m.precision = prec
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(T(x[k]))
    m = m.cuda()
    m.train(train)
    q = T(x["q"]).cuda().requires_grad_(True)
    k = q if form == "qkv" else T(x["k"]).cuda().requires_grad_(True)
    v = k if form != "sep" else T(x["v"]).cuda().requires_grad_(True)
    mask = None if attn_mask(c) is None else T(attn_mask(c)).cuda()
    bias = None if learned_bias(c) is None else T(learned_bias(c)).cuda().requires_grad_(True)
    kpm = T(padding(c)).cuda()
    return m, dict(q=q, k=k, v=v, w=T(x["w"]).cuda(), mask=mask, bias=bias, kpm=kpm)


def step(m, a, need_weights=True, **over):
    """One forward + backward from clean gradients -> {name: tensor}; over: replacements of the call's arguments."""
    a = dict(a, **over)
    q, k, v, bias = a["q"], a["k"], a["v"], a["bias"]
    for t in [q, k, v, bias] + list(m.parameters()):
        if t is not None:
            t.grad = None
    y, wt = m(q, k, v, attn_mask=a["mask"], need_weights=need_weights, attn_bias=bias, key_padding_mask=a["kpm"])
    (y * a["w"]).sum().backward()
    torch.cuda.synchronize()
    out = {"attn": y.detach(), "weights": wt, "gq": q.grad.clone()}
    if k is not q:
        out["gk"] = k.grad.clone()
    if v is not k:
        out["gv"] = v.grad.clone()
    for n, p in m.named_parameters():
        out["g." + n] = p.grad.clone()
    if bias is not None and bias.requires_grad:
        out["g.bias"] = bias.grad.clone()
    return out


def compare(prec, tag, name, a, ref):
    """a, ref: numpy arrays of one shape."""
    assert a.shape == ref.shape, (tag, name, a.shape, ref.shape)
    assert np.isfinite(a).all(), (tag, name)
    scale = max(1.0, float(np.abs(ref).max()))
    err = float(np.abs(a - ref).max())
    rel = float(np.linalg.norm((a - ref).ravel()) / max(np.linalg.norm(ref.ravel()), 1e-6))
    _note(prec, tag, name, rel, err)
    print(f"{prec} {tag}.{name}: max err {err:.3e} (scale {scale:.3g}), rel-L2 {rel:.3e}")
    if prec == "f32":
        assert err <= F32_LIMIT * scale, f"{tag}.{name}: max err {err:.3e} > {F32_LIMIT * scale:.3e}"
    else:
        lim = KPM_BF16_LIMIT[kind_of(name)]
        assert rel <= lim and err <= 4 * lim * scale, f"{tag}.{name}: rel-L2 {rel:.3e} (limit {lim:.1e}), max err {err:.3e} (scale {scale:.3g})"


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_module_matches_the_reference(tag, prec):
    c = case(tag)
    m, a = build(c, prec)
    got = step(m, a)
    if tag in REFERENCE_RUNS:
        names = sorted(n[len(tag) + 1:] for n in G if n.startswith(tag + ".") and not n.endswith((".idx", ".n")))
        assert sorted(got) == names, (sorted(got), names)
        for name in names:
            key = f"{tag}.{name}"
            x = got[name].detach().float().cpu().numpy()
            idx = G.get(key + ".idx")
            if idx is not None:
                x = np.take(x, idx, axis=1 if name == "weights" else 0)
            compare(prec, tag, name, x, G[key])
    else:
        ref = restate(c)
        assert sorted(got) == sorted(ref)
        for name in sorted(ref):
            compare(prec, tag, name, got[name].detach().float().cpu().numpy(), ref[name].numpy())
    # exact: padded keys
    pm = padding(c)                                                           # [B, S]
    wn = got["weights"].cpu().numpy()
    assert (wn[np.broadcast_to(pm[:, None, :], wn.shape)] == 0).all(), "weights at a padded key must be exactly 0"
    assert (wn[~visible(c).any(1)] == 0).all(), "weights at a pair hidden in every head must be exactly 0"
    assert float(np.abs(wn.astype(np.float64).sum(-1) - 1).max()) <= (2e-5 if prec == "f32" else 1.5e-2)
    if c[1] in ("kv", "sep"):
        for n in ("gk", "gv"):
            if n in got:
                assert (got[n].cpu().numpy()[pm.T] == 0).all(), f"{n} rows of padded positions must be exactly 0"
    if "g.bias" in got:
        g = got["g.bias"].cpu().numpy()
        assert g.shape == learned_bias(c).shape and (g[np.isinf(learned_bias(c))] == 0).all()
        g3 = g if g.ndim == 3 else g[None]
        assert (g3[~visible(c).any(0)] == 0).all(), "no gradient at a pair hidden in every sample"
    assert a["kpm"].grad is None


def test_an_edited_padding_mask_is_read_again_and_leaves_the_additive_image_alone():
    c = case("k3")
    m, a = build(c, "f32")
    first = step(m, a)
    image, kbytes = m._exec._mask, m._exec._kmask
    assert image is not None and kbytes is not None
    again = step(m, a)
    assert m._exec._kmask is kbytes and m._exec._mask is image, "an unchanged mask reuses the cached bytes"
    assert torch.equal(again["attn"], first["attn"])
    a["kpm"][0, 60:] = True                                                   # in place: sample 0 loses its tail
    edited = step(m, a)
    assert m._exec._kmask is not kbytes, "an edited mask must be read again"
    assert m._exec._mask is image, "the additive image does not depend on the padding mask"
    assert not torch.equal(edited["attn"][:, 0], first["attn"][:, 0]) and torch.equal(edited["attn"][:, 1:], first["attn"][:, 1:])
    assert float(edited["weights"][0, :, 60:].abs().max()) == 0.0
    fresh = step(m, a, kpm=a["kpm"].clone())                                  # another tensor with the same values
    assert m._exec._mask is image
    assert torch.equal(fresh["attn"], edited["attn"]) and torch.equal(fresh["g.bias"], edited["g.bias"])
    as_bytes = step(m, a, kpm=a["kpm"].to(torch.uint8) * 7)                   # uint8, any nonzero value means padding
    assert torch.equal(as_bytes["attn"], edited["attn"]) and torch.equal(as_bytes["gk"], edited["gk"])


@pytest.mark.parametrize("tag", ["k1", "k4"])
def test_dropout_in_training_is_reproducible_per_seed(tag):
    c = case(tag)
    m, a = build(c, "bf16", dropout=0.1, train=True)
    torch.manual_seed(5)
    m._step = 0
    x = step(m, a)
    y = step(m, a)                                                            # the next call draws another mask
    assert not torch.equal(x["attn"], y["attn"])
    torch.manual_seed(5)
    m._step = 0
    z = step(m, a)
    for n in x:
        same = torch.allclose(x[n], z[n], rtol=1e-5, atol=1e-5 * float(z[n].abs().max())) if n.endswith("proj_bias") or n == "g.out_proj.bias" \
            else torch.equal(x[n], z[n])                 # the projection-bias gradients are column sums by float atomics
        assert same, n
    pm = padding(c)
    assert (x["gk"].cpu().numpy()[pm.T] == 0).all() and float(x["weights"].cpu().numpy()[np.broadcast_to(pm[:, None, :], x["weights"].shape)].max()) == 0.0


@pytest.mark.parametrize("how", ["transposed", "sliced"])
def test_a_mask_with_strides_of_its_own_is_read_as_its_contiguous_twin(how):
    """key_padding_mask as a transposed [S, B] tensor (what `(tokens == pad).t()` gives for time-major tokens) or as every
    second column of a wider one: the same bits as its .contiguous() copy, weights exactly 0 at the padded keys."""
    c = case("k3")
    m, a = build(c, "bf16")
    pm = a["kpm"]
    B, S = pm.shape
    if how == "transposed":
        odd = pm.t().contiguous().t()                                         # strides (1, B)
    else:
        wide = torch.ones(B, 2 * S, dtype=torch.bool, device="cuda")
        wide[:, ::2] = pm
        odd = wide[:, ::2]                                                    # strides (2 S, 2)
    assert not odd.is_contiguous() and torch.equal(odd, pm)
    x = step(m, a, kpm=odd)
    y = step(m, a, kpm=odd.contiguous())
    for n in x:
        same = torch.allclose(x[n], y[n], rtol=1e-5, atol=1e-5 * float(y[n].abs().max())) if n.endswith("proj_bias") or n == "g.out_proj.bias" \
            else torch.equal(x[n], y[n])
        assert same, n
    w = x["weights"].cpu().numpy()
    assert (w[np.broadcast_to(padding(c)[:, None, :], w.shape)] == 0).all(), "weights at a padded key must be exactly 0"
    assert (x["gk"].cpu().numpy()[padding(c).T] == 0).all()


def _spy(monkeypatch):
    """Every ops.attn_* launch wrapper records its name before running."""
    calls = []
    for name in dir(ops):
        fn = getattr(ops, name)
        if name.startswith("attn_") and callable(fn) and ("fwd" in name or "bwd" in name or "maps" in name) and "ws_bytes" not in name:
            def wrap(*a_, _fn=fn, _name=name, **k_):
                calls.append(_name + ("+kmasks" if k_.get("kmasks") is not None else ""))
                return _fn(*a_, **k_)
            monkeypatch.setattr(ops, name, wrap)
    return calls


def test_each_combination_launches_its_own_family(monkeypatch):
    c = case("k4")
    m, a = build(c, "bf16")
    calls = _spy(monkeypatch)
    step(m, a, kpm=None, mask=None, bias=None)
    assert calls == ["attn_fwd", "attn_maps", "attn_bwd_dq", "attn_bwd_dkv"], calls
    del calls[:]
    step(m, a, kpm=None)                                                      # today's entries: no _kmask / _kamask call
    assert calls == ["attn_fwd_amask", "attn_maps_amask", "attn_bwd_dq_amask", "attn_bwd_dkv_amask", "attn_bwd_dbias"], calls
    del calls[:]
    step(m, a, mask=None, bias=None)                                          # a padding mask alone: no _amask entry
    assert calls == ["attn_fwd_kmask", "attn_maps_kmask", "attn_bwd_dq_kmask", "attn_bwd_dkv_kmask"], calls
    del calls[:]
    step(m, a)
    assert calls == ["attn_fwd_kamask", "attn_maps_kamask", "attn_bwd_dq_kamask", "attn_bwd_dkv_kamask", "attn_bwd_dbias+kmasks"], calls
    del calls[:]
    step(m, a, bias=a["bias"].detach())                                       # a bias without grad: no dbias entry
    assert calls == ["attn_fwd_kamask", "attn_maps_kamask", "attn_bwd_dq_kamask", "attn_bwd_dkv_kamask"], calls
    del calls[:]
    out = step(m, a, need_weights=False)                                      # no maps entry
    assert out["weights"] is None
    assert calls == ["attn_fwd_kamask", "attn_bwd_dq_kamask", "attn_bwd_dkv_kamask", "attn_bwd_dbias+kmasks"], calls


def test_without_a_padding_mask_the_bits_are_todays(monkeypatch):
    """key_padding_mask=None and an all-False mask give the same result bit for bit (all-ones bytes: the *_hmask bits)."""
    c = case("k3")
    m, a = build(c, "f32")
    x = step(m, a, kpm=None)
    y = step(m, a, kpm=torch.zeros_like(a["kpm"]))
    for n in x:
        same = torch.allclose(x[n], y[n], rtol=1e-5, atol=1e-5 * float(y[n].abs().max())) if n.endswith("proj_bias") or n == "g.out_proj.bias" \
            else torch.equal(x[n], y[n])
        assert same, n


def test_refusals_on_the_device():
    c = case("k2")
    m, a = build(c, "f32")
    q = a["q"]
    with pytest.raises(ValueError, match="key_padding_mask on cpu, the inputs on cuda"):
        m(q, q, q, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match="key_padding_mask of shape"):
        m(q, q, q, key_padding_mask=torch.zeros(2, 6, dtype=torch.bool, device="cuda"))
    with pytest.raises(ValueError, match="key_padding_mask must be"):
        m(q, q, q, key_padding_mask=torch.zeros(2, 5, device="cuda"))
    m.precision = "bf16x3"
    with pytest.raises(ValueError, match="bf16x3"):
        m(q, q, q, key_padding_mask=a["kpm"])
