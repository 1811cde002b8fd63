#!/usr/bin/env python3
"""Generate the encoder padding-mask fixture encoder_kpm.npz from the REAL reference TransformerEncoder on the CPU, in
train mode with every dropout rate 0, with the harness of make_golden.py (imported, not changed).  The reference has no
padding mask but is independent across samples, so it runs one sample at a time (B = 1 slices of the inputs).  In this
process only, every layer gets attn_mask = True and bpmult.models.transformer.buffered_future_mask is replaced by a
function of our own, which returns the case's rule (the future mask of tests/encoder_kpm_cases.py, or zeros) with -inf in
the columns the current sample's padding hides: `tensor2 is None` is the self-attention call (encoder_padding_mask), a
second tensor the cross-attention call (key_padding_mask) -- transformer.py:155-166.  Outputs and input gradients are
concatenated over the batch; the parameter gradients accumulate over the samples' backward passes.

Per case `tag`: "<tag>.y", "<tag>.gx", "<tag>.gkv" (cross forms: d(x_in_k) + d(x_in_v), one tensor passed as both) and
"<tag>.g.<parameter>" for every parameter the reference gives a gradient.

usage:  python tests/golden/make_golden_encoder_kpm.py
"""
import os
import sys

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
import make_golden as mg  # noqa: E402  (applies the reference shims)
from encoder_kpm_cases import CASES, LAYERS, blocks, inputs, param, rule  # noqa: E402

torch, tr = mg.torch, mg.tr
_NOW = {}            # the sample being run: {"self": additive [T, T], "cross": additive [T, S]}


def _mask(tensor, tensor2=None):
    m = _NOW["self" if tensor2 is None else "cross"]
    assert m.shape == (tensor.size(0), (tensor if tensor2 is None else tensor2).size(0))
    return m


tr.buffered_future_mask = _mask


def encoder_kpm():
    out = {}

    def put(key, t):
        assert torch.isfinite(t).all(), f"{key}: the reference produced a non-finite value"
        out[key] = t.detach().numpy()

    for c in CASES:
        tag, form, bi, Tn, S, B, d, H = c[:8]
        m = tr.TransformerEncoder(d, H, LAYERS, attn_mask=True, biprojection=bi)
        for layer in m.layers:
            layer.attn_mask = True                     # the rule itself (causal or none) comes from _mask
        with torch.no_grad():
            for k, p in m.named_parameters():
                p.copy_(mg.T(param(c, k, p.shape)))
        m.train()                                      # all dropout rates are 0
        x = inputs(c)
        ys, gxs, gkvs = [], [], []
        for b in range(B):
            _NOW.clear()
            for blk, pm in blocks(c):
                add = rule(c, blk).copy()
                if pm is not None:
                    add[:, pm[b]] = -np.inf
                _NOW[blk] = mg.T(add)
            xb = mg.T(x["x"][:, b:b + 1].copy()).requires_grad_(True)
            if form == "cross":
                kvb = mg.T(x["kv"][:, b:b + 1].copy()).requires_grad_(True)
                y = m(xb, kvb, kvb)
            else:
                y = m(xb)
            (y * mg.T(x["w"][:, b:b + 1].copy())).sum().backward()
            ys.append(y.detach()), gxs.append(xb.grad)
            if form == "cross":
                gkvs.append(kvb.grad)
        put(f"{tag}.y", torch.cat(ys, 1))
        put(f"{tag}.gx", torch.cat(gxs, 1))
        if form == "cross":
            put(f"{tag}.gkv", torch.cat(gkvs, 1))
        for k, p in m.named_parameters():
            if p.grad is not None:
                put(f"{tag}.g.{k}", p.grad)
    mg.save("encoder_kpm", **out)


if __name__ == "__main__":
    torch.set_num_threads(8)
    print("encoder_kpm")
    encoder_kpm()
