#!/usr/bin/env python3
"""Generate the self-attention-stack fixture F15 from the REAL reference TransformerEncoder.forward(x) (no key / value
source), with the harness of make_golden.py (its shims, deterministic weights / inputs and fixture layout; that file is
imported, not changed).  B = 2, the last two time steps zero-padded, some channel-0 entries zeroed (as F5).

  case  layer kind     d    heads (head_dim)  layers  T    mask
  sb    biprojection   24   4 (6)             2       7    on    (FFN on layer_norms.2; layer_norms.1 gets no gradient)
  sn    plain          24   4 (6)             2       9    off
  s25   plain          50   2 (25 -> 32)      2       70   on    (crosses a 64-row tile)
  s128  plain          256  2 (128)           2       130  on
  s256  biprojection   512  2 (256)           1       40   on

Per case: y and gx at the time steps "rows" -- every one for T <= 70; for the two wide cases every fourth (tile edges
0 / 64 / 128 included) and the last, which keeps the file near the size of the other fixtures -- with the norm and sum of
the whole tensors ("yn", "gxn"); for every parameter its gradient norm and sum ("gn." + name, float64); full gradients
("g." + name) of the parameters with at most 4096 elements; the names without a gradient ("nograd").

usage:  python tests/golden/make_golden_self_attn.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the reference shims)

CASES = (("sb", True, 24, 4, 2, 7, True), ("sn", False, 24, 4, 2, 9, False), ("s25", False, 50, 2, 2, 70, True),
         ("s128", False, 256, 2, 2, 130, True), ("s256", True, 512, 2, 1, 40, True))
B = 2
FULL_MAX = 4096


def f15_self_encoder():
    out = {}
    for tag, bi, d, H, Ly, Tn, mask in CASES:
        pfx = f"f15{tag}."
        m = mg.tr.TransformerEncoder(d, H, Ly, attn_mask=mask, biprojection=bi)
        mg.load_det(m, pfx)
        m.train()
        x = mg.zero_some_channel0(mg.T(mg.det(pfx + "x", (Tn, B, d))), pfx + "x")
        with mg.torch.no_grad():
            x[-2:] = 0.0                                       # zero-padded tail rows
        x.requires_grad_(True)
        y = m(x)
        (y * mg.T(mg.det(pfx + "w", y.shape))).sum().backward()
        rows = np.arange(Tn) if Tn <= 70 else np.array(sorted(set(range(0, Tn, 4)) | {Tn - 1}))
        for nm, t in (("y", y.detach()), ("gx", x.grad)):
            out[f"{tag}.{nm}"] = t.numpy()[rows]
            out[f"{tag}.{nm}n"] = np.array([t.double().norm().item(), t.double().sum().item()])
        out[f"{tag}.rows"] = rows
        nograd = []
        for k, p in m.named_parameters():
            if p.grad is None:
                nograd.append(k)
                continue
            g = p.grad.double()
            out[f"{tag}.gn.{k}"] = np.array([g.norm().item(), g.sum().item()])
            if p.numel() <= FULL_MAX:
                out[f"{tag}.g.{k}"] = p.grad.numpy()
        out[f"{tag}.nograd"] = np.array(nograd, dtype=str)
    mg.save("f15_self_encoder", **out)


if __name__ == "__main__":
    mg.torch.set_num_threads(8)
    print("f15")
    f15_self_encoder()
