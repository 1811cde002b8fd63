#!/usr/bin/env python3
"""Generate the per-head attention-map fixture head_maps.npz from the REAL reference: the [B*H, T, S] softmax
probabilities its MultiheadAttention forms internally (multihead_attention.py:121) before it averages them over the heads
(:133-134), all dropout rates 0.  The reference never returns that tensor, so it is captured where the module computes it:
for the time of this process the name `F` that multihead_attention.py calls `F.softmax` through is a proxy that forwards
everything to torch.nn.functional and keeps a copy of each softmax result (nothing of torch is changed, nothing is
written back).  A forward hook on the same attention module pairs each captured tensor with the call's second return
value and asserts that its head mean IS that value, bit for bit; the outputs are asserted bit-equal to the stored F5 / F15 /
F16 / F7 / mha_kpm fixtures, so the new arrays belong to what the existing tests pin.  Uses the harness of make_golden.py
(imported, not changed), as make_golden_attn_maps.py does.

Standalone encoders, full maps [B, H, T, S] under "<case>.L<layer>.<block>" (block "self" / "cross"):
  x, xn, x25, b            the F5 cases
  sb                       one self-attention case of F15 (biprojection layers called as forward(x))
  c130x70, c128, c256      of F16
The F7 model (mmtrvat, d 24, 4 heads, 2 layers, 512 x 512 maps), per encoder and layer "m.<encoder>.L<layer>":
  ".hn"    float64 [H, 2]: (norm, sum) of every head's map, all twelve encoders
  ".rows"  the query rows ROWS of every head in full, [B, H, 8, 512], for the two encoders FULL
MultiheadAttention: "mha.<tag>" [B, H, T, S] for the three REFERENCE_RUNS of tests/mha_kpm_cases.py, run one sample at a
time with the padding folded into attn_mask exactly as make_golden_mha_kpm.py runs them.

usage:  python tests/golden/make_golden_head_maps.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (applies the reference shims)
import make_golden_attn_maps as mga  # noqa: E402
import make_golden_self_attn as mgs  # noqa: E402
from mha_kpm_cases import CASES as KPM_CASES, REFERENCE_RUNS, additive, inputs, padding  # noqa: E402

torch = mg.torch
B = 2
ROWS = mga.ROWS
FULL = ("trans_l_with_a", "trans_a_with_v2l")          # one encoder of each level
F15_CASE = "sb"
F16_CASES = ("c130x70", "c128", "c256")
LIMIT_BYTES = 1500 * 1000

_CAPTURED = []


class _Functional:
    """torch.nn.functional as multihead_attention.py sees it: softmax also keeps its result."""

    def __init__(self, real):
        self._real = real

    def __getattr__(self, name):
        return getattr(self._real, name)

    def softmax(self, *a, **k):
        p = self._real.softmax(*a, **k)
        _CAPTURED.append(p.detach().clone())
        return p


_mha_module = sys.modules[mg.MHA.__module__]
_mha_module.F = _Functional(_mha_module.F)


def hook_heads(attn, sink, key):
    """Forward hook on one MultiheadAttention: sink[key] collects, per call, the probabilities [B, H, T, S] the call formed."""
    def keep(mod, inp, out):
        (p,) = _CAPTURED                            # exactly one softmax per call
        del _CAPTURED[:]
        w = out[1].detach()
        bsz = w.shape[0]
        p = p.view(bsz, mod.num_heads, *p.shape[1:])
        assert torch.equal(p.sum(dim=1) / mod.num_heads, w), f"{key}: the head mean is not the module's second return value"
        sink.setdefault(key, []).append((p, w))
    return attn.register_forward_hook(keep)


def encoder_case(out, avg, pfx, tag, bi, d, H, Ly, Tn, S, mask, check_y):
    m = mg.tr.TransformerEncoder(d, H, Ly, attn_mask=mask, biprojection=bi)
    mg.load_det(m, pfx)
    m.train()
    x = mg.zero_some_channel0(mg.T(mg.det(pfx + "x", (Tn, B, d))), pfx + "x")
    with torch.no_grad():
        x[-2:] = 0.0
    sink = {}
    for i, layer in enumerate(m.layers):
        hook_heads(layer.self_attn, sink, i)
    with torch.no_grad():
        if S:
            kv = mg.zero_some_channel0(mg.T(mg.det(pfx + "kv", (S, B, d))), pfx + "kv")
            y = m(x, kv, kv)
        else:
            y = m(x)
    check_y(y)
    for i in range(Ly):
        calls = sink[i]
        blocks = ("self", "cross") if len(calls) == 2 else (("cross",) if S else ("self",))
        assert len(calls) == len(blocks), (tag, i, len(calls))
        for blk, (p, w) in zip(blocks, calls):
            assert tuple(p.shape) == (B, H, Tn, Tn if blk == "self" else S), (tag, blk, p.shape)
            assert np.array_equal(w.numpy(), avg[f"{tag}.L{i}.{blk}"]), f"{tag}.L{i}.{blk}: head mean differs from f16_attn_maps.npz"
            out[f"{tag}.L{i}.{blk}"] = p.numpy()


def model_case(out, avg):
    pfx = "f7."
    torch.manual_seed(0)
    args = mg._args(hidden_sz=24, num_heads=4, layers=2, orig_d_l=32)
    model = mg.mmtr.MultiprojectionMMTransformer3DGMUClf(args)
    model.train()                                          # all dropout rates are 0
    mg.load_det(model, pfx)
    xl = mg.T(mg.det(pfx + "xl", (B, 50, 32)))
    img, aud = mg.T(mg.det(pfx + "img", (B, 500, 35))), mg.T(mg.det(pfx + "aud", (B, 375, 74)))
    model.enc.feat = xl
    sink = {}
    names = [n for n, mod in model.named_children() if n.startswith("trans_") and hasattr(mod, "layers")]
    assert names == avg["m.names"].tolist() and all(n in names for n in FULL), names
    for n in names:
        for i, layer in enumerate(getattr(model, n).layers):
            hook_heads(layer.self_attn, sink, (n, i))
    with torch.no_grad():
        logits, _ = model(None, None, None, img, aud, output_gate=True)
    stored = np.load(os.path.join(HERE, "f7_mmtrvat.npz"))["logits"]
    assert np.array_equal(logits.numpy(), stored), "mmtrvat: logits differ from f7_mmtrvat.npz"
    out["m.names"] = np.array(names, dtype=str)
    out["m.full"] = np.array(FULL, dtype=str)
    out["m.query_rows"] = ROWS
    for n in names:
        for i in range(2):
            ((p, w),) = sink[(n, i)]
            assert tuple(p.shape) == (B, 4, 512, 512)
            key = f"m.{n}.L{i}"
            assert np.array_equal(w.numpy()[:, ROWS], avg[key + ".rows"]), f"{key}: head mean differs from f16_attn_maps.npz"
            pd = p.double()
            out[key + ".hn"] = np.stack([pd.pow(2).sum(dim=(0, 2, 3)).sqrt().numpy(), pd.sum(dim=(0, 2, 3)).numpy()], axis=1)
            if n in FULL:
                out[key + ".rows"] = p.numpy()[:, :, ROWS]


def mha_cases(out):
    stored = np.load(os.path.join(HERE, "mha_kpm.npz"))
    for c in KPM_CASES:
        tag, form, Tn, S, Bn, d, H, _, learned, bias, _ = c
        if tag not in REFERENCE_RUNS:
            continue
        m = mg.MHA(d, H, bias=bias)
        mg.load_det(m, tag + ".")
        m.eval()
        sink = {}
        hook_heads(m, sink, tag)
        x, pm, (eff,) = inputs(c), padding(c), additive(c)
        ys = []
        with torch.no_grad():
            for b in range(Bn):
                q = mg.T(x["q"][:, b:b + 1].copy())
                k = q if form == "qkv" else mg.T(x["k"][:, b:b + 1].copy())
                mask_b = eff.copy()
                mask_b[:, pm[b]] = -np.inf
                y, _ = m(q, k, k, attn_mask=mg.T(mask_b))
                ys.append(y)
        y, w = torch.cat(ys, 1), torch.cat([w for _, w in sink[tag]], 0)
        for name, t in (("attn", y), ("weights", w)):       # the stored fixture keeps (norm, sum) of the whole tensors
            n = np.array([t.double().norm().item(), t.double().sum().item()])
            assert np.array_equal(n, stored[f"{tag}.{name}.n"]), f"{tag}.{name}: differs from mha_kpm.npz"
        p = torch.cat([p for p, _ in sink[tag]], 0)
        assert tuple(p.shape) == (Bn, H, Tn, S)
        assert (p.numpy()[np.broadcast_to(pm[:, None, None, :], p.shape)] == 0).all()
        out[f"mha.{tag}"] = p.numpy()


def head_maps():
    out = {}
    avg = np.load(os.path.join(HERE, "f16_attn_maps.npz"))
    f5 = np.load(os.path.join(HERE, "f5_encoder.npz"))
    f15 = np.load(os.path.join(HERE, "f15_self_encoder.npz"))

    def equals(stored):
        def check(y):
            assert np.array_equal(y.numpy(), stored), "output differs from the stored fixture"
        return check

    def norm_equals(stored):
        def check(y):
            assert np.array_equal(np.array([y.double().norm().item(), y.double().sum().item()]), stored), "output norm / sum differ"
        return check

    for tag, bi, d, H, Ly, Tn, S, mask in mga.F5_CASES:
        encoder_case(out, avg, f"f5{tag}.", tag, bi, d, H, Ly, Tn, S, mask, equals(f5[f"{tag}.y"]))
    (tag, bi, d, H, Ly, Tn, mask), = [c for c in mgs.CASES if c[0] == F15_CASE]

    def f15_check(y):
        assert np.array_equal(y.numpy()[f15[f"{tag}.rows"]], f15[f"{tag}.y"]) and \
            np.array_equal(np.array([y.double().norm().item(), y.double().sum().item()]), f15[f"{tag}.yn"]), "output differs from f15_self_encoder.npz"
    encoder_case(out, avg, f"f15{tag}.", tag, bi, d, H, Ly, Tn, 0, mask, f15_check)
    for tag, bi, d, H, Ly, Tn, S, mask in mga.NEW_CASES:
        if tag in F16_CASES:
            encoder_case(out, avg, f"f16{tag}.", tag, bi, d, H, Ly, Tn, S, mask, norm_equals(avg[f"{tag}.yn"]))
    model_case(out, avg)
    mha_cases(out)
    mg.save("head_maps", **out)
    size = os.path.getsize(os.path.join(HERE, "head_maps.npz"))
    assert size <= LIMIT_BYTES, f"head_maps.npz is {size} bytes"


if __name__ == "__main__":
    torch.set_num_threads(8)
    print("head maps")
    head_maps()
