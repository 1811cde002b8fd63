#!/usr/bin/env python3
"""Generate the MultiheadAttention module fixture mha.npz from the REAL reference MultiheadAttention.forward(query, key,
value, attn_mask) on the CPU, in eval mode, with the harness of make_golden.py (its shims -- the in_proj_qkv clone that the
in-place `q *= self.scaling` needs under autograd --, deterministic weights / inputs and fixture layout; that file is
imported, not changed).  The cases and the masks are in tests/mha_cases.py.

Per case `tag`: "<tag>.attn", "<tag>.weights" (head-averaged, [B, T, S]), the input gradients "<tag>.gq" (and ".gk", ".gv"
where key / value are tensors of their own) and the parameter gradients "<tag>.g.<name>" under the upstream gradient
det("<tag>.w").  Tensors above mha_cases.THIN_ABOVE elements are stored as every fourth slice (and the last) with the
index array "<key>.idx"; "<key>.n" holds the norm and the sum of the whole tensor (float64) for every key.

usage:  python tests/golden/make_golden_mha.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (applies the reference shims)
from mha_cases import CASES, make_mask, thin  # noqa: E402


def mha():
    out = {}

    def put(tag, name, t):
        a = t.detach().numpy()
        key = f"{tag}.{name}"
        idx, part = thin(name, a)
        out[key] = part
        if idx is not None:
            out[key + ".idx"] = idx
        out[key + ".n"] = np.array([t.detach().double().norm().item(), t.detach().double().sum().item()])

    for tag, form, Tn, S, B, d, H, kind, bias in CASES:
        pfx = tag + "."
        m = mg.MHA(d, H, bias=bias)
        mg.load_det(m, pfx)
        m.eval()
        q = mg.leaf(pfx + "q", (Tn, B, d))
        if form == "qkv":
            k = v = q
        elif form == "kv":
            k = v = mg.leaf(pfx + "k", (S, B, d))
        else:
            k, v = mg.leaf(pfx + "k", (S, B, d)), mg.leaf(pfx + "v", (S, B, d))
        mask = make_mask(kind, Tn, S, pfx)
        if kind == "future":
            ref_mask = mg.tr.buffered_future_mask(q, k)
            assert np.array_equal(ref_mask.numpy(), mask), "mha_cases.make_mask('future') != buffered_future_mask"
        y, w = m(q, k, v, attn_mask=None if mask is None else mg.T(mask))
        (y * mg.T(mg.det(pfx + "w", y.shape))).sum().backward()
        put(tag, "attn", y)
        put(tag, "weights", w)
        put(tag, "gq", q.grad)
        if form == "kv":
            put(tag, "gk", k.grad)
        elif form == "sep":
            put(tag, "gk", k.grad)
            put(tag, "gv", v.grad)
        for name, p in m.named_parameters():
            put(tag, "g." + name, p.grad)
    mg.save("mha", **out)


if __name__ == "__main__":
    mg.torch.set_num_threads(8)
    print("mha")
    mha()
