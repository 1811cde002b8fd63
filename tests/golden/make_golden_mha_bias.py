#!/usr/bin/env python3
"""Generate the learned-attention-bias fixture mha_bias.npz from the REAL reference MultiheadAttention.forward(query, key,
value, attn_mask=mask.requires_grad_()) on the CPU, in eval mode, with the harness of make_golden.py (imported, not
changed) and the masks of tests/mha_cases.py: `attn_weights += attn_mask.unsqueeze(0)` is an ordinary autograd op, so
mask.grad is the gradient a learned [T, S] bias receives.  The cases are in tests/mha_bias_cases.py.

Per case `tag`: "<tag>.attn", "<tag>.weights" (head-averaged, [B, T, S]), the input gradients "<tag>.gq" (and ".gk"), the
parameter gradients "<tag>.g.<name>" and "<tag>.g.bias" = mask.grad under the upstream gradient det("<tag>.w"); thinned and
summarised ("<key>.idx", "<key>.n") as make_golden_mha.py does.

usage:  python tests/golden/make_golden_mha_bias.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (applies the reference shims)
from mha_cases import thin  # noqa: E402
from mha_bias_cases import CASES, shared_bias  # noqa: E402


def mha_bias():
    out = {}

    def put(tag, name, t):
        a = t.detach().numpy()
        key = f"{tag}.{name}"
        idx, part = thin(name, a)
        out[key] = part
        if idx is not None:
            out[key + ".idx"] = idx
        out[key + ".n"] = np.array([t.detach().double().norm().item(), t.detach().double().sum().item()])

    for c in CASES:
        tag, form, Tn, S, B, d, H, kind, bias = c
        pfx = tag + "."
        m = mg.MHA(d, H, bias=bias)
        mg.load_det(m, pfx)
        m.eval()
        q = mg.leaf(pfx + "q", (Tn, B, d))
        k = v = q if form == "qkv" else mg.leaf(pfx + "k", (S, B, d))
        mask = mg.T(shared_bias(c)).requires_grad_()
        y, w = m(q, k, v, attn_mask=mask)
        (y * mg.T(mg.det(pfx + "w", y.shape))).sum().backward()
        g = mask.grad
        hidden = np.isinf(shared_bias(c))
        assert np.isfinite(g.numpy()).all() and (g.numpy()[hidden] == 0).all() and float(g.sum(-1).abs().max()) <= 2e-6
        put(tag, "attn", y)
        put(tag, "weights", w)
        put(tag, "gq", q.grad)
        if form == "kv":
            put(tag, "gk", k.grad)
        for name, p in m.named_parameters():
            put(tag, "g." + name, p.grad)
        put(tag, "g.bias", g)
    mg.save("mha_bias", **out)


if __name__ == "__main__":
    mg.torch.set_num_threads(8)
    print("mha_bias")
    mha_bias()
