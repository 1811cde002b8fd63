#!/usr/bin/env python3
"""Generate the key_padding_mask fixture mha_kpm.npz from the REAL reference MultiheadAttention on the CPU, in eval mode,
with the harness of make_golden.py (imported, not changed).  The reference has no key_padding_mask argument but is
independent across samples, so it runs one sample at a time (B = 1 slices of the inputs): sample b gets
attn_mask = (the case's additive image, or 0) with -inf in the columns key_padding_mask[b] hides -- with requires_grad_()
where the case learns a bias: `attn_weights += attn_mask.unsqueeze(0)` is an ordinary autograd op, so mask.grad, summed
over the samples, is the gradient of the bias.  attn, weights and the input gradients are concatenated over the batch;
the parameter gradients accumulate over the samples' backward passes.  The cases are in tests/mha_kpm_cases.py (those of
REFERENCE_RUNS: an [H, T, S] bias cannot run in the reference).

Per case `tag`: "<tag>.attn", "<tag>.weights" ([B, T, S]), "<tag>.gq" (and ".gk"), "<tag>.g.<name>" and, with a learned
bias, "<tag>.g.bias"; thinned and summarised ("<key>.idx", "<key>.n") as make_golden_mha.py does.

usage:  python tests/golden/make_golden_mha_kpm.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (applies the reference shims)
from mha_cases import thin  # noqa: E402
from mha_kpm_cases import CASES, REFERENCE_RUNS, additive, inputs, padding  # noqa: E402

torch = mg.torch


def mha_kpm():
    out = {}

    def put(tag, name, t):
        assert torch.isfinite(t).all(), f"{tag}.{name}: the reference produced a non-finite value"
        a = t.detach().numpy()
        key = f"{tag}.{name}"
        idx, part = thin(name, a)
        out[key] = part
        if idx is not None:
            out[key + ".idx"] = idx
        out[key + ".n"] = np.array([t.detach().double().norm().item(), t.detach().double().sum().item()])

    for c in CASES:
        tag, form, Tn, S, B, d, H, _, learned, bias, _ = c
        if tag not in REFERENCE_RUNS:
            continue
        assert form in ("qkv", "kv") and learned in (None, "shared")
        m = mg.MHA(d, H, bias=bias)
        mg.load_det(m, tag + ".")
        m.eval()
        x, pm, (eff,) = inputs(c), padding(c), additive(c)
        ys, ws, gqs, gks, gbias = [], [], [], [], torch.zeros(Tn, S)
        for b in range(B):
            q = mg.T(x["q"][:, b:b + 1].copy()).requires_grad_(True)
            k = q if form == "qkv" else mg.T(x["k"][:, b:b + 1].copy()).requires_grad_(True)
            mask_b = eff.copy()
            mask_b[:, pm[b]] = -np.inf
            mask = mg.T(mask_b)
            if learned:
                mask.requires_grad_()
            y, w = m(q, k, k, attn_mask=mask)
            (y * mg.T(x["w"][:, b:b + 1].copy())).sum().backward()
            ys.append(y.detach()), ws.append(w.detach()), gqs.append(q.grad)
            if form == "kv":
                gks.append(k.grad)
            if learned:
                assert (mask.grad.numpy()[np.isinf(mask_b)] == 0).all()
                gbias += mask.grad
        put(tag, "attn", torch.cat(ys, 1))
        put(tag, "weights", torch.cat(ws, 0))
        put(tag, "gq", torch.cat(gqs, 1))
        if form == "kv":
            put(tag, "gk", torch.cat(gks, 1))
        for name, p in m.named_parameters():
            put(tag, "g." + name, p.grad)
        if learned:
            put(tag, "g.bias", gbias)
    mg.save("mha_kpm", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    print("mha_kpm")
    mha_kpm()
