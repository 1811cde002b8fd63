"""Cases of the learned-attention-bias fixture (tests/golden/mha_bias.npz), shared by its generator
(tests/golden/make_golden_mha_bias.py, which runs the reference with attn_mask=mask.requires_grad_()) and the tests, and an
fp64 torch restatement of the module for the form the reference cannot run (an [H, T, S] bias: its in-place add rejects
the broadcast).  Inputs, weights, the upstream gradient and the biases are regenerated from names by detgen.

  case  call form    T    S   B  d    H  dh  bias kind                                  in/out-proj bias
  b1    k is v       65   67  2  128  2  64  mixed (finite values with -inf holes)      yes
  b2    q is k is v  5    5   2  50   2  25  finite                                     no
  b3    k is v       130  67  3  64   2  32  mixed                                      yes
"""
import numpy as np
import torch

from detgen import det, det_param
from mha_cases import make_mask

# tag, call form, T, S, B, d, H, bias kind, in/out-projection bias
CASES = (("b1", "kv", 65, 67, 2, 128, 2, "mixed", True),
         ("b2", "qkv", 5, 5, 2, 50, 2, "finite", False),
         ("b3", "kv", 130, 67, 3, 64, 2, "mixed", True))
PARAMS = ("in_proj_weight", "in_proj_bias", "out_proj.weight", "out_proj.bias")


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def shared_bias(c):
    """float32 [T, S]: the mask of mha_cases under the case's prefix (what the fixture's reference run was given)."""
    tag, _, T, S, _, _, _, kind, _ = c
    return make_mask(kind, T, S, tag + ".")


def head_bias(c):
    """float32 [H, T, S]: one image per head, each with its own values and its own -inf pattern."""
    tag, _, T, S, _, _, H, kind, _ = c
    return np.stack([make_mask(kind, T, S, f"{tag}.h{h}.") for h in range(H)])


def inputs(c):
    """name -> float32 numpy: the parameters the case has, q (and k, v where they are tensors of their own), w."""
    tag, form, T, S, B, d, H, _, bias = c
    pfx = tag + "."
    out = {"in_proj_weight": det_param(pfx + "in_proj_weight", (3 * d, d)), "out_proj.weight": det_param(pfx + "out_proj.weight", (d, d))}
    if bias:
        out["in_proj_bias"] = det_param(pfx + "in_proj_bias", (3 * d,))
        out["out_proj.bias"] = det_param(pfx + "out_proj.bias", (d,))
    out["q"] = det(pfx + "q", (T, B, d))
    if form != "qkv":
        out["k"] = det(pfx + "k", (S, B, d))
    if form == "sep":
        out["v"] = det(pfx + "v", (S, B, d))
    out["w"] = det(pfx + "w", (T, B, d))
    return out


def restate(c, bias, mask=None, table=None):
    """The module in fp64 torch: in-projection, scale, scores + bias (+ mask), softmax, P V, out-projection; autograd for
    every gradient under the upstream gradient w.  bias: float32 numpy [T, S] or [H, T, S]; or, with `table` (a float32
    numpy vector), an integer numpy index array of one of those shapes: the bias is table[bias] and the table gets the
    gradient.  Returns {name: float64 tensor} with the fixture's names: attn, weights, gq (gk, gv), g.<parameter>, g.bias
    (g.table)."""
    tag, form, T, S, B, d, H, _, _ = c
    dh = d // H
    x = {k: torch.from_numpy(v).double() for k, v in inputs(c).items()}
    leaves = {k: x[k].clone().requires_grad_(True) for k in x if k != "w"}
    q = leaves["q"]
    k = leaves.get("k", q)
    v = leaves.get("v", k)
    if table is None:
        b = torch.from_numpy(bias).double().requires_grad_(True)
        eff = b
    else:
        b = torch.from_numpy(table).double().requires_grad_(True)
        eff = b[torch.from_numpy(bias)]
    W, ib = leaves["in_proj_weight"], leaves.get("in_proj_bias")

    def proj(t, i):
        y = t @ W[i * d:(i + 1) * d].t()
        if ib is not None:
            y = y + ib[i * d:(i + 1) * d]
        return y.reshape(t.shape[0], B, H, dh).permute(1, 2, 0, 3)          # [B, H, L, dh]

    sc = (proj(q, 0) * dh ** -0.5) @ proj(k, 1).transpose(-1, -2) + eff      # [T, S] and [H, T, S] both broadcast over [B, H, T, S]
    if mask is not None:
        sc = sc + torch.from_numpy(mask).double()
    pr = torch.softmax(sc, -1)
    o = (pr @ proj(v, 2)).permute(2, 0, 1, 3).reshape(T, B, d)
    y = o @ leaves["out_proj.weight"].t()
    if "out_proj.bias" in leaves:
        y = y + leaves["out_proj.bias"]
    (y * x["w"]).sum().backward()
    out = {"attn": y.detach(), "weights": pr.detach().mean(1), "gq": q.grad}
    if k is not q:
        out["gk"] = k.grad
    if v is not k:
        out["gv"] = v.grad
    for n in PARAMS:
        if n in leaves:
            out["g." + n] = leaves[n].grad
    out["g.table" if table is not None else "g.bias"] = b.grad
    return out
