"""TransformerEncoder's padding masks (encoder_padding_mask / key_padding_mask) on the MI355X, in all three layer kinds and
both call forms: forward, backward and attention_maps().

Parity: cases e1 - e5 of tests/encoder_kpm_cases.py against the REAL reference's sample-by-sample run
(tests/golden/encoder_kpm.npz, make_golden_encoder_kpm.py), output, input gradients and every parameter gradient, compared
as test_encoder_gpu.py::close does:
  f32, bf16x3  max error <= 2e-4 of max(1, |ref|max), the project's limit
  bf16         relative L2 error per case and kind of tensor <= 2x the error measured on the MI355X (BF16_MEASURED below,
               profiles/encoder_kpm_errors.json), and max error <= 4x the F5 limit of the kind (F5_LIMIT) of the scale
Independence of the padding's content: bit for bit.  Hidden keys: probability, map weight and gradient exactly 0."""
import json
import os

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import bpmult_amd  # noqa: E402,F401
from bpmult_amd.models.encoder import TransformerEncoder  # noqa: E402
from encoder_kpm_cases import CASES, LAYERS, case, inputs, padding, param  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
TOL = 2e-4
# the limits of test_encoder_gpu.py (F5) per kind of tensor: a measured bf16 error above them would be a finding
F5_LIMIT = {"y": 1e-2, "gx": 1e-1, "gkv": 1e-1, "weight": 1.4e-1, "bias": 1.4e-1, "layer_norm": 2e-1}
# bf16: the largest relative L2 error per case and kind of tensor measured on the MI355X against the fixture (rounded up
# to two digits; profiles/encoder_kpm_errors.json, "bf16.*"); the limit is 2x
BF16_MEASURED = {
    "e1": {"y": 0.00080, "gx": 0.0038, "gkv": 0.0058, "weight": 0.030, "bias": 0.033, "layer_norm": 0.033},
    "e2": {"y": 0.00044, "gx": 0.0042, "gkv": 0.0062, "weight": 0.039, "bias": 0.038, "layer_norm": 0.056},
    "e3": {"y": 0.0011, "gx": 0.0015, "gkv": 0.0069, "weight": 0.0084, "bias": 0.0038, "layer_norm": 0.0088},
    "e4": {"y": 0.00072, "gx": 0.0047, "weight": 0.027, "bias": 0.025, "layer_norm": 0.037},
    "e5": {"y": 0.00070, "gx": 0.0081, "weight": 0.055, "bias": 0.047, "layer_norm": 0.053},
}
_MEASURED = {}
# where the measured errors go (the JSON of profiles/encoder_kpm_errors.json): set BPMULT_ERROR_LOG to a file path to record
# them; unset, nothing is written
_LOG = os.environ.get("BPMULT_ERROR_LOG")
_FIX = {}


def fixture():
    if not _FIX:
        _FIX.update(np.load(os.path.join(G, "encoder_kpm.npz")))
    return _FIX


def kind(what):
    return what if what in ("y", "gx", "gkv") else "layer_norm" if "layer_norm" in what else "bias" if "bias" in what else "weight"


def _note(prec, tag, what, err):
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
    """Appends a failure to `bad` (every tensor of a case is measured, and printed, before the test fails)."""
    a = a.detach().float().cpu().numpy()
    assert a.shape == b.shape, (what, a.shape, b.shape)
    assert np.isfinite(a).all(), what
    scale = max(1.0, float(np.abs(b).max()))
    err = float(np.abs(a - b).max())
    if prec == "bf16":
        rel = float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-6))
        _note(prec, tag, what, rel)
        print(f"{prec} {tag} {what}: rel-L2 {rel:.3e}, max err {err:.3e} (scale {scale:.3g})")
        lim, f5 = 2.0 * BF16_MEASURED[tag][kind(what)], F5_LIMIT[kind(what)]
        if rel > lim or err > 4 * f5 * scale:
            bad.append(f"{what}: rel-L2 {rel:.3e} (limit {lim:.2e}), max err {err:.3e} (limit {4 * f5 * scale:.2e})")
    else:
        _note(prec, tag, what, err / scale)
        print(f"{prec} {tag} {what}: max err {err:.3e} (scale {scale:.3g})")
        if err > TOL * scale:
            bad.append(f"{what}: max err {err:.3e} > {TOL * scale:.3e}")


def make(c, prec, **kw):
    tag, _, bi, _, _, _, d, H, causal = c[:9]
    enc = TransformerEncoder(d, H, LAYERS, attn_mask=causal, biprojection=bi, **kw)
    enc.precision = prec
    with torch.no_grad():
        for k, p in enc.named_parameters():
            p.copy_(T(param(c, k, p.shape)))
    return enc.cuda().train()


def masks(c, as_bytes=False):
    """The call's keyword arguments: bool masks, or (as_bytes) uint8 masks that are strided views of larger tensors."""
    out = {}
    for name, pm in zip(("encoder_padding_mask", "key_padding_mask"), padding(c)):
        if pm is None:
            continue
        m = T(pm).cuda()
        if as_bytes:
            wide = torch.full((m.shape[0], 2 * m.shape[1] + 1), 7, dtype=torch.uint8, device="cuda")
            wide[:, 1::2] = m.to(torch.uint8) * 3              # nonzero = padding, whatever the value
            m = wide[:, 1::2]
            assert not m.is_contiguous()
        out[name] = m
    return out


def run(c, enc, x, kv=None, w=None, **mk):
    """One forward + backward through the module -> {"y", "gx", "gkv" (cross forms), "g.<parameter>"} (device tensors)."""
    I = inputs(c)
    for p in enc.parameters():
        p.grad = None
    x = (T(I["x"]) if x is None else x).cuda().requires_grad_(True)
    w = (T(I["w"]) if w is None else w).cuda()
    if c[1] == "cross":
        kv = (T(I["kv"]) if kv is None else kv).cuda().requires_grad_(True)
        y = enc(x, kv, kv, **mk)
    else:
        y = enc(x, **mk)
    (y * w).sum().backward()
    out = {"y": y.detach(), "gx": x.grad}
    if kv is not None:
        out["gkv"] = kv.grad
    for k, p in enc.named_parameters():
        out["g." + k] = p.grad
    return out


PARITY = [(c[0], prec) for c in CASES for prec in ("f32", "bf16")] + [("e3", "bf16x3")]


@pytest.mark.parametrize("tag,prec", PARITY, ids=[f"{t}-{p}" for t, p in PARITY])
def test_against_the_reference(tag, prec):
    c, g = case(tag), fixture()
    enc = make(c, prec)
    got = run(c, enc, None, **masks(c, as_bytes=prec == "bf16"))
    bad = []
    for name in ("y", "gx") + (("gkv",) if c[1] == "cross" else ()):
        close(got[name], g[f"{tag}.{name}"], prec, name, tag, bad)
    for k, _ in enc.named_parameters():
        if f"{tag}.g.{k}" not in g:                      # layer_norms.1 of the biprojection self-attention stack: unused there
            assert c[2] and c[1] == "self" and "layer_norms.1." in k, k
            assert got["g." + k] is None or not bool(got["g." + k].any()), k
            continue
        assert got["g." + k] is not None, k
        close(got["g." + k], g[f"{tag}.g.{k}"], prec, k, tag, bad)
    assert not bad, bad


def test_measured_bf16_errors_stay_below_the_f5_limits():
    for tag, per in BF16_MEASURED.items():
        for k, v in per.items():
            assert v <= F5_LIMIT[k], (tag, k)


# --- independence of the padding's content ---------------------------------------------------------------------------------
def _same_bits(a, b, what):
    assert a.dtype == b.dtype and a.shape == b.shape, what
    assert torch.equal(a, b), f"{what}: {int((a != b).sum())} of {a.numel()} elements differ, max {float((a - b).abs().max()):.3e}"


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_padded_key_rows_do_not_reach_the_result(prec):
    """e2: the padded rows of x_in_k filled with other finite values."""
    c = case("e2")
    _, kpm = padding(c)
    pad = T(kpm.T.copy()).cuda()                                               # [S, B]
    enc = make(c, prec)
    base = run(c, enc, None, **masks(c))
    kv = T(inputs(c)["kv"].copy())
    other = T(np.random.default_rng(5).standard_normal(kv.shape).astype(np.float32)) * 3
    kv[pad.cpu()] = other[pad.cpu()]
    alt = run(c, enc, None, kv=kv, **masks(c))
    assert bool(pad.any()) and bool((~pad).any())
    for k in base:
        if k == "gkv":
            for r in (base, alt):
                assert bool((r["gkv"][pad] == 0).all()), "d(key source) of a padded position is exactly 0"
            _same_bits(base["gkv"][~pad], alt["gkv"][~pad], "gkv on the real rows")
        else:
            _same_bits(base[k], alt[k], k)
    assert bool(torch.isfinite(alt["y"]).all())


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_padded_query_rows_do_not_reach_the_real_rows(prec):
    """e4 (self-attention stack): the padded rows of x_in changed, the upstream gradient 0 on those rows."""
    c = case("e4")
    epm, _ = padding(c)
    pad = T(epm.T.copy())                                                      # [T, B]
    I = inputs(c)
    w = T(I["w"].copy())
    w[pad] = 0.0
    x = T(I["x"].copy())
    other = T(np.random.default_rng(6).standard_normal(x.shape).astype(np.float32)) * 3
    x2 = x.clone()
    x2[pad] = other[pad]
    enc = make(c, prec)
    base = run(c, enc, x, w=w, **masks(c))
    alt = run(c, enc, x2, w=w, **masks(c))
    pad = pad.cuda()
    for k in base:
        if k in ("y", "gx"):
            _same_bits(base[k][~pad], alt[k][~pad], f"{k} on the real rows")
        else:
            _same_bits(base[k], alt[k], k)
    for r in (base, alt):
        assert bool((r["gx"][pad] == 0).all()), "d(x_in) of a padded row with no upstream gradient is exactly 0"
        assert bool(torch.isfinite(r["y"]).all())
    assert not torch.equal(base["y"][pad], alt["y"][pad]), "the padded rows themselves are computed like any other row"


def test_hidden_keys_get_no_gradient_under_dropout():
    """e1 in training with every dropout rate 0.5: the exact zeros do not depend on the dropout masks."""
    c = case("e1")
    _, kpm = padding(c)
    pad = T(kpm.T.copy()).cuda()
    enc = make(c, "bf16", attn_dropout=0.5, relu_dropout=0.5, res_dropout=0.5, embed_dropout=0.5)
    got = run(c, enc, None, **masks(c))
    assert all(bool(torch.isfinite(v).all()) for v in got.values())
    assert bool((got["gkv"][pad] == 0).all()) and bool((got["gkv"][~pad] != 0).any())
    enc.eval()
    assert float((run(c, enc, None, **masks(c))["y"] - got["y"]).abs().max()) > 1e-2, "dropout must be active in train mode"


def test_mask_content_changes_between_calls_of_one_plan():
    """The plan's tables are fixed; every forward refills its visibility buffers: masks A, then masks B, then none, on one
    module equal a fresh module's run with each."""
    c = case("e3")
    enc = make(c, "f32")
    a = masks(c)
    b = {k: torch.flip(v, dims=(0,)) for k, v in a.items()}                    # the samples' paddings swapped
    none = {}
    first = run(c, enc, None, **a)
    for mk in (b, none, a):
        got, want = run(c, enc, None, **mk), run(c, make(c, "f32"), None, **mk)
        for k in want:
            # two modules: the limit of test_self_encoder_gpu.py::test_one_module_called_both_ways (a stale mask is O(1) off)
            assert float((got[k] - want[k]).abs().max()) <= 1e-6 * max(1.0, float(want[k].abs().max())), k
    assert not torch.equal(first["y"], run(c, enc, None, **b)["y"])
    assert len(enc._plans) == 2, "one plan for the masked calls, one for the call without masks"


# --- maps ------------------------------------------------------------------------------------------------------------------
def test_attention_maps_are_taken_under_the_masks():
    c = case("e3")
    tag, _, _, Tn, S, B = c[:6]
    epm, kpm = padding(c)
    enc = make(c, "f32")
    I = inputs(c)
    x, kv = T(I["x"]).cuda().requires_grad_(True), T(I["kv"]).cuda()
    y = enc(x, kv, kv, **masks(c))
    maps = enc.attention_maps()
    assert len(maps) == LAYERS
    for per in maps:
        assert set(per) == {"self", "cross"}
        for name, pm, n in (("self", epm, Tn), ("cross", kpm, S)):
            W = per[name].weights
            assert W.shape == (B, Tn, n) and W.dtype == torch.float32 and per[name].query_steps is None
            hid = T(np.broadcast_to(pm[:, None, :], (B, Tn, n)).copy()).cuda()
            assert bool((W[hid] == 0).all()), f"{name}: a padded key has weight exactly 0"
            assert float((W.sum(-1) - 1).abs().max()) <= 1e-5, name
            # the future-mask rule still holds beside the padding (mask_off 1 / 4)
            i, j = torch.arange(Tn, device="cuda")[:, None], torch.arange(n, device="cuda")[None, :]
            assert bool((W[:, j - i >= 1 + abs(n - Tn)] == 0).all()), name
            assert bool((W[~hid & (j - i < 1 + abs(n - Tn))[None].expand(B, Tn, n)] > 0).all()), name
    (y * T(I["w"]).cuda()).sum().backward()                                    # valid until the next forward, backward or not
    again = enc.attention_maps([1])
    for name in ("self", "cross"):
        _same_bits(again[0][name].weights, maps[1][name].weights, name)
