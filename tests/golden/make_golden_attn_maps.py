#!/usr/bin/env python3
"""Generate the attention-map fixture F16 from the REAL reference: the second return value of every
`layers[i].self_attn` call (multihead_attention.py:132-135, the softmax probabilities averaged over the heads, [B, T, S]),
taken by forward hooks, all dropout rates 0.  Uses the harness of make_golden.py (its shims, deterministic weights / inputs
and fixture layout; that file is imported, not changed).

Standalone encoders (full maps, key "<case>.L<layer>.<block>", block = "self" or "cross"; a biprojection layer with a
key / value source calls its attention twice: self, then cross):
  x, xn, x25, b          the F5 cases, rebuilt exactly as make_golden.f5_encoder does
  sb, sn, s25, s128, s256  the F15 cases (forward(x)), rebuilt exactly as make_golden_self_attn does
     -- the generator asserts that the output y it gets equals the stored y of f5_encoder.npz / f15_self_encoder.npz bit for
     bit: the maps belong to the outputs the existing tests pin.
  c130x70, c70x130       crossmodal, d 50 / 2 heads (head_dim 25 -> 32), 2 layers, T x S = 130 x 70 and 70 x 130, mask on
  c128                   crossmodal, d 256 / 2 heads (head_dim 128), 1 layer, 70 x 40, mask on
  c256                   biprojection, d 512 / 2 heads (head_dim 256), 1 layer, 40 x 70, mask on
     (B = 2, inputs and weights by name as F5: prefix "f16<case>."; "<case>.yn" = float64 norm and sum of the output)

One whole model, `mmtrvat` at F7's configuration (d 24, 4 heads, 2 layers, B 2, 50 / 500 / 375 -> 512), logits asserted
bit-equal to f7_mmtrvat.npz.  Per encoder and layer ("m.<encoder>.L<layer>"): the query rows ROWS of the 512 x 512 map in
full (".rows": [B, 8, 512]) and float64 (norm, sum) of the whole map and of map * det("f16m.w.<encoder>.L<layer>")
(".n", ".wn").

usage:  python tests/golden/make_golden_attn_maps.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the reference shims)
import make_golden_self_attn as mgs  # noqa: E402

torch = mg.torch
B = 2
ROWS = np.array([0, 1, 63, 64, 255, 256, 510, 511])
# (case, biprojection, d, heads, layers, T, S, mask)
F5_CASES = (("x", False, 24, 4, 2, 7, 5, True), ("xn", False, 24, 4, 2, 6, 6, False), ("x25", False, 50, 2, 2, 8, 11, True),
            ("b", True, 24, 4, 2, 5, 8, True))
NEW_CASES = (("c130x70", False, 50, 2, 2, 130, 70, True), ("c70x130", False, 50, 2, 2, 70, 130, True),
             ("c128", False, 256, 2, 1, 70, 40, True), ("c256", True, 512, 2, 1, 40, 70, True))


def hook_maps(encoder, sink, name):
    """Forward hooks on every layers[i].self_attn of `encoder`: sink[(name, i)] collects the weights of each call."""
    hs = []
    for i, layer in enumerate(encoder.layers):
        def keep(mod, inp, out, i=i):
            sink.setdefault((name, i), []).append(out[1].detach().clone())
        hs.append(layer.self_attn.register_forward_hook(keep))
    return hs


def encoder_case(out, pfx, tag, bi, d, H, Ly, Tn, S, mask, stored_y=None):
    m = mg.tr.TransformerEncoder(d, H, Ly, attn_mask=mask, biprojection=bi)
    mg.load_det(m, pfx)
    m.train()
    x = mg.zero_some_channel0(mg.T(mg.det(pfx + "x", (Tn, B, d))), pfx + "x")
    with torch.no_grad():
        x[-2:] = 0.0
    sink = {}
    hook_maps(m, sink, tag)
    with torch.no_grad():
        if S:
            kv = mg.zero_some_channel0(mg.T(mg.det(pfx + "kv", (S, B, d))), pfx + "kv")
            y = m(x, kv, kv)
        else:
            y = m(x)
    if stored_y is not None:
        assert np.array_equal(y.numpy(), stored_y), f"{tag}: output differs from the stored fixture"
    else:
        out[f"{tag}.yn"] = np.array([y.double().norm().item(), y.double().sum().item()])
    for i in range(Ly):
        calls = sink[(tag, i)]
        blocks = ("self", "cross") if len(calls) == 2 else (("cross",) if S else ("self",))
        assert len(calls) == len(blocks), (tag, i, len(calls))
        for blk, w in zip(blocks, calls):
            assert tuple(w.shape) == (B, Tn, Tn if blk == "self" else S), (tag, blk, w.shape)
            out[f"{tag}.L{i}.{blk}"] = w.numpy()


def model_case(out):
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
    assert len(names) == 12, names
    for n in names:
        hook_maps(getattr(model, n), sink, n)
    with torch.no_grad():
        logits, _ = model(None, None, None, img, aud, output_gate=True)
    stored = np.load(os.path.join(HERE, "f7_mmtrvat.npz"))["logits"]
    assert np.array_equal(logits.numpy(), stored), "mmtrvat: logits differ from f7_mmtrvat.npz"
    out["m.names"] = np.array(names, dtype=str)
    out["m.query_rows"] = ROWS
    for n in names:
        for i in range(2):
            (w,) = sink[(n, i)]
            assert tuple(w.shape) == (B, 512, 512)
            key = f"m.{n}.L{i}"
            wd = w.double()
            det_w = mg.T(mg.det(f"f16m.w.{n}.L{i}", tuple(w.shape))).double()
            out[key + ".rows"] = w.numpy()[:, ROWS]
            out[key + ".n"] = np.array([wd.norm().item(), wd.sum().item()])
            out[key + ".wn"] = np.array([(wd * det_w).norm().item(), (wd * det_w).sum().item()])


def f16_attn_maps():
    out = {}
    f5 = np.load(os.path.join(HERE, "f5_encoder.npz"))
    f15 = np.load(os.path.join(HERE, "f15_self_encoder.npz"))
    for tag, bi, d, H, Ly, Tn, S, mask in F5_CASES:
        encoder_case(out, f"f5{tag}.", tag, bi, d, H, Ly, Tn, S, mask, stored_y=f5[f"{tag}.y"])
    for tag, bi, d, H, Ly, Tn, mask in mgs.CASES:
        y15 = f15[f"{tag}.y"]
        rows = f15[f"{tag}.rows"]
        sub = {}
        encoder_case(sub, f"f15{tag}.", tag, bi, d, H, Ly, Tn, 0, mask, stored_y=None)
        # F15 stores y at the time steps "rows" plus the norm / sum of the whole tensor: both must match bit for bit
        m = mg.tr.TransformerEncoder(d, H, Ly, attn_mask=mask, biprojection=bi)
        mg.load_det(m, f"f15{tag}.")
        m.train()
        x = mg.zero_some_channel0(mg.T(mg.det(f"f15{tag}.x", (Tn, B, d))), f"f15{tag}.x")
        with torch.no_grad():
            x[-2:] = 0.0
            y = m(x)
        assert np.array_equal(y.numpy()[rows], y15), f"{tag}: output differs from f15_self_encoder.npz"
        assert np.array_equal(sub.pop(f"{tag}.yn"), f15[f"{tag}.yn"]), f"{tag}: output norm / sum differ from f15_self_encoder.npz"
        out.update(sub)
    for tag, bi, d, H, Ly, Tn, S, mask in NEW_CASES:
        encoder_case(out, f"f16{tag}.", tag, bi, d, H, Ly, Tn, S, mask)
    model_case(out)
    mg.save("f16_attn_maps", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    print("f16")
    f16_attn_maps()
