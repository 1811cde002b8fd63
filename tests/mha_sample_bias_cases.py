"""Cases of the per-sample attention masks and biases of MultiheadAttention (tests/test_mha_sample_bias_cpu.py,
tests/test_mha_sample_bias_module_gpu.py), in the pattern of tests/mha_bias_cases.py with B >= 2 and B != H, so that sample
and head cannot be confused.  The reference cannot run these forms (its in-place `+= attn_mask.unsqueeze(0)` rejects the
broadcast): the oracle is mha_bias_cases.restate, whose bias broadcasts over [B, H, T, S].

  case  call form    T    S   B  d    H  dh  bias kind   in/out-proj bias
  s1    k is v       65   67  3  128  2  64  mixed       yes
  s2    q is k is v  5    5   3  50   2  25  finite      no
  s3    k is v       130  67  3  64   2  32  mixed       yes
"""
import numpy as np

from mha_cases import make_mask

CASES = (("s1", "kv", 65, 67, 3, 128, 2, "mixed", True),
         ("s2", "qkv", 5, 5, 3, 50, 2, "finite", False),
         ("s3", "kv", 130, 67, 3, 64, 2, "mixed", True))
FORMS = ("B1TS", "(BH)TS")        # attn_bias forms (the 4-D [B, H, T, S] spelling stays refused for a bias); "BHTS": masks only


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def sample_bias(c, form):
    """float32 numpy in `form`: one image per sample ([B, 1, T, S]) or per sample and head ([B, H, T, S]; "(BH)TS": the same
    flattened to torch's [B*H, T, S], index b*H + h), each with its own values and its own -inf pattern."""
    tag, _, T, S, B, _, H, kind, _ = c
    Hm = 1 if form == "B1TS" else H
    m = np.stack([np.stack([make_mask(kind, T, S, f"{tag}.b{b}.h{h}.") for h in range(Hm)]) for b in range(B)])
    return m.reshape(B * H, T, S) if form == "(BH)TS" else m


def as4(c, a):
    """an image of any accepted form as [Bm, Hm, T, S] (what restate broadcasts)"""
    _, _, T, S, B, _, H, _, _ = c
    if a.ndim == 2:
        return a[None, None]
    if a.ndim == 3:
        return a[None] if a.shape[0] == H else a.reshape(B, H, T, S)
    return a


def shared_mask(c):
    """float32 [T, S], finite: a mask beside the bias"""
    tag, _, T, S = c[:4]
    return make_mask("finite", T, S, tag + ".mask.")
