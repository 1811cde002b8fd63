"""Cases of the key_padding_mask fixture (tests/golden/mha_kpm.npz), shared by its generator
(tests/golden/make_golden_mha_kpm.py) and the tests.  The reference's MultiheadAttention has no key_padding_mask argument
but is independent across samples: the generator runs it one sample at a time with the padding folded into attn_mask as
-inf columns.  An fp64 torch restatement of the module (mha_bias_cases.restate with the padding as a per-sample additive
term) stands in for the form the reference cannot run (k4: an [H, T, S] bias -- its in-place add rejects the broadcast).
Inputs, weights, the upstream gradient, the masks and the biases are regenerated from names by detgen.

  case  call form      T    S   B  d    H  dh  additive                                              padded keys per sample
  k1    k is v         65   67  3  128  2  64  none                                                  none / [40,67) / [0,64)
  k2    q is k is v    5    5   2  50   2  25  finite attn_mask, no in/out-projection bias           none / [3,5)
  k3    k is v         130  67  3  64   2  32  learned [T,S] bias: finite values with -inf holes     none / [50,67) / [0,64)
  k4    three tensors  65   67  2  192  2  96  finite attn_mask AND learned [H,T,S] bias with holes  [64,67) / [0,1)

The smallest shapes that cross a 64-key tile, hide a whole tile (the last sample of k1 and k3: the first tile, for every
row) and leave a ragged tail.  Holes: det > 0.2533 (P = 0.4), columns i % 50 and 64 + i % 3 of row i kept finite, so every
(sample, query row) keeps a visible key under padding and holes together -- asserted below, at import.
"""
import numpy as np

import mha_bias_cases as mb
from detgen import det

NINF = np.float32(-np.inf)
# tag, call form, T, S, B, d, H, attn_mask kind (None / "finite"), learned bias (None / "shared" / "heads"),
# in/out-projection bias, padded key range [lo, hi) per sample (None: no padding)
CASES = (("k1", "kv", 65, 67, 3, 128, 2, None, None, True, (None, (40, 67), (0, 64))),
         ("k2", "qkv", 5, 5, 2, 50, 2, "finite", None, False, (None, (3, 5))),
         ("k3", "kv", 130, 67, 3, 64, 2, None, "shared", True, (None, (50, 67), (0, 64))),
         ("k4", "sep", 65, 67, 2, 192, 2, "finite", "heads", True, ((64, 67), (0, 1))))
REFERENCE_RUNS = ("k1", "k2", "k3")        # the cases of the fixture


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def padding(c):
    """bool [B, S]: True marks a padded key (the key_padding_mask argument)."""
    S, B, pads = c[3], c[4], c[10]
    pm = np.zeros((B, S), dtype=bool)
    for b, r in enumerate(pads):
        if r is not None:
            pm[b, r[0]:r[1]] = True
    return pm


def attn_mask(c):
    """float32 [T, S], finite, or None."""
    tag, T, S, kind = c[0], c[2], c[3], c[7]
    return None if kind is None else det(f"{tag}.mask.f", (T, S), 2.0)


def _holes(pfx, T, S):
    hidden = det(pfx + "bias.u", (T, S)) > 0.2533
    rows = np.arange(T)
    hidden[rows, rows % 50] = False
    hidden[rows, 64 + rows % 3] = False
    return np.where(hidden, NINF, det(pfx + "bias.f", (T, S), 2.0)).astype(np.float32)


def learned_bias(c):
    """float32 [T, S] ("shared") or [H, T, S] ("heads", each head its own values and holes), or None."""
    tag, T, S, H, kind = c[0], c[2], c[3], c[6], c[8]
    if kind is None:
        return None
    if kind == "shared":
        return _holes(tag + ".", T, S)
    return np.stack([_holes(f"{tag}.h{h}.", T, S) for h in range(H)])


def additive(c):
    """float32 [Hm, T, S] (Hm 1 or H): attn_mask + learned bias, zeros when the case has neither."""
    T, S = c[2], c[3]
    eff = np.zeros((1, T, S), dtype=np.float32)
    m, b = attn_mask(c), learned_bias(c)
    if m is not None:
        eff = eff + m
    if b is not None:
        eff = eff + (b if b.ndim == 3 else b[None])
    return eff.astype(np.float32)


def visible(c):
    """bool [B, Hm, T, S]: the pairs that padding and holes leave."""
    return ~padding(c)[:, None, None, :] & np.isfinite(additive(c))[None]


def bias_case(c):
    """The case as mha_bias_cases spells one (its inputs() / restate() read tag, form, sizes and the projection bias)."""
    tag, form, T, S, B, d, H = c[:7]
    return (tag, form, T, S, B, d, H, None, c[9])


def inputs(c):
    return mb.inputs(bias_case(c))


def restate(c):
    """The module in fp64 torch (mha_bias_cases.restate): the padding enters as a per-sample additive [B, 1, T, S] term of
    0 / -inf beside attn_mask.  {name: float64 tensor} with the fixture's names; g.bias only where the case learns one."""
    T, S, B = c[2], c[3], c[4]
    per_sample = np.zeros((B, 1, T, S), dtype=np.float32)
    per_sample[np.broadcast_to(padding(c)[:, None, None, :], per_sample.shape)] = NINF
    m = attn_mask(c)
    if m is not None:
        per_sample = per_sample + m
    b = learned_bias(c)
    out = mb.restate(bias_case(c), np.zeros((T, S), dtype=np.float32) if b is None else b, mask=per_sample)
    if b is None:
        del out["g.bias"]
    return out


# condition, not measurement: every (sample, head image, query row) keeps at least one visible key
for _c in CASES:
    _v = visible(_c)
    assert _v.any(-1).all(), f"{_c[0]}: a query row lost all its keys"
    assert padding(_c).shape == (_c[4], _c[3])
assert visible(case("k3")).sum(-1).min() == 1, "k3 is the case with a single visible key in some row"
assert not visible(case("k3"))[2, :, :, :64].any() and not visible(case("k1"))[2, :, :, :64].any(), "a wholly hidden first tile"
