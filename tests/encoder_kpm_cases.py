"""Cases of the encoder padding-mask fixture (tests/golden/encoder_kpm.npz), shared by its generator
(tests/golden/make_golden_encoder_kpm.py) and the tests.  The reference's TransformerEncoder has no padding mask (its
docstrings promise an encoder_padding_mask, transformer.py:62-63, and never implement one) but is independent across
samples: the generator runs it one sample at a time with the padding folded into the layers' attn_mask as -inf columns.
Inputs, weights and the upstream gradient are regenerated from names by detgen; every case has 2 layers.

  case  call form  kind          T   S   B  d / H              rule                  padded ranges per sample
  e1    x, k, v    crossmodal    7   9   3  24 / 4             causal (mask_off 3)   keys: none, [6,9), [1,9) (row 0 keeps one key)
  e2    x, k, v    crossmodal    8   70  3  50 / 2 (dh 25)     none                  keys: [64,70) (a whole tail tile), [0,64) (a whole
                                                                                     first tile), none
  e3    x, k, v    biprojection  8   5   2  24 / 4             causal (mask_off 4)   rows of x: none, [5,8); keys: [3,5), none
  e4    x          plain         9   -   3  24 / 4             causal                rows: none, [5,9), [1,9)
  e5    x          biprojection  66  -   2  24 / 4             none                  rows: [64,66), [0,64)

The smallest shapes at which the engine's wiring can go wrong (which block reads which mask, in which layer kind and call
form, forward, backward and maps); the kernels themselves are covered by test_attn_kmask_gpu.py.
"""
import numpy as np

from detgen import det, det_param

NINF = np.float32(-np.inf)
LAYERS = 2
# tag, call form ("cross": forward(x, k, v); "self": forward(x)), biprojection, T, S (None: no key source), B, d, H,
# attn_mask (the causal rule), padded ranges [lo, hi) of x_in's rows per sample (None: no encoder_padding_mask; an entry
# None: that sample has no padding), padded ranges of the key source's rows (None: no key_padding_mask)
CASES = (("e1", "cross", False, 7, 9, 3, 24, 4, True, None, (None, (6, 9), (1, 9))),
         ("e2", "cross", False, 8, 70, 3, 50, 2, False, None, ((64, 70), (0, 64), None)),
         ("e3", "cross", True, 8, 5, 2, 24, 4, True, (None, (5, 8)), ((3, 5), None)),
         ("e4", "self", False, 9, None, 3, 24, 4, True, (None, (5, 9), (1, 9)), None),
         ("e5", "self", True, 66, None, 2, 24, 4, False, ((64, 66), (0, 64)), None))


def case(tag):
    return next(c for c in CASES if c[0] == tag)


def pfx(c):
    return f"ekpm.{c[0]}."


def _pad(ranges, B, n):
    if ranges is None:
        return None
    pm = np.zeros((B, n), dtype=bool)
    for b, r in enumerate(ranges):
        if r is not None:
            pm[b, r[0]:r[1]] = True
    return pm


def padding(c):
    """(encoder_padding_mask bool [B, T] or None, key_padding_mask bool [B, S] or None): True marks a padded row."""
    _, _, _, T, S, B, _, _, _, rows, keys = c
    return _pad(rows, B, T), _pad(keys, B, S)


def rule(c, block):
    """float32 [T, n] (n = T for block "self", S for "cross"): the reference's buffered_future_mask of the block under
    attn_mask=True (transformer.py:209-216: -inf where j - i >= 1 + |n - T|), zeros without it."""
    T, S, causal = c[3], c[4], c[8]
    n = T if block == "self" else S
    m = np.zeros((T, n), dtype=np.float32)
    if causal:
        i, j = np.arange(T)[:, None], np.arange(n)[None, :]
        m[j - i >= 1 + abs(n - T)] = NINF
    return m


def blocks(c):
    """The attention blocks the case's call runs, each with its padding mask (or None): [(block, bool [B, n] or None)]."""
    form, bi = c[1], c[2]
    epm, kpm = padding(c)
    out = []
    if form == "self" or bi:
        out.append(("self", epm))
    if form == "cross":
        out.append(("cross", kpm))
    return out


def visible(c, block, pm):
    """bool [B, T, n]: the (sample, query row, key) triples that rule and padding leave."""
    r = np.isfinite(rule(c, block))[None]
    B = c[5]
    hid = np.zeros((B, 1, r.shape[2]), dtype=bool) if pm is None else pm[:, None, :]
    return np.broadcast_to(r, (B,) + r.shape[1:]) & ~hid


def _zero_some_channel0(x, name):
    """A few channel-0 entries exactly 0, so that the reference's padding-position rule fires (make_golden.py)."""
    m = det(name + ".z", x.shape[:2]) > 1.0
    x[:, :, 0][m] = 0.0
    return x


def inputs(c):
    """{"x": [T, B, d], "kv": [S, B, d] (cross forms), "w": upstream gradient [T, B, d]}, float32."""
    _, form, _, T, S, B, d, _, _, _, _ = c
    p = pfx(c)
    out = {"x": _zero_some_channel0(det(p + "x", (T, B, d)), p + "x"), "w": det(p + "w", (T, B, d))}
    if form == "cross":
        out["kv"] = _zero_some_channel0(det(p + "kv", (S, B, d)), p + "kv")
    return out


def param(c, name, shape):
    return det_param(pfx(c) + name, shape)


# conditions, not measurements: every (sample, query row) of every block keeps a visible key under rule and padding
# together, and e1 has a row that keeps exactly one
for _c in CASES:
    for _blk, _pm in blocks(_c):
        assert visible(_c, _blk, _pm).any(-1).all(), f"{_c[0]}: a query row of the {_blk} block lost all its keys"
    assert any(pm is not None for _, pm in blocks(_c)), f"{_c[0]}: no block reads a mask"
assert visible(case("e1"), "cross", padding(case("e1"))[1]).sum(-1).min() == 1, "e1 is the case with a single visible key in some row"
