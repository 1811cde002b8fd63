"""Cases of the MultiheadAttention module fixture (tests/golden/mha.npz), shared by its generator
(tests/golden/make_golden_mha.py, which runs the reference) and tests/test_mha_module_gpu.py.  Inputs, weights, the
upstream gradient and the masks are regenerated from names by detgen on both sides; the fixture carries only outputs.

  case  call form      T    S    B  d    H  dh  mask                                    bias
  m1    q is k is v    65   65   3  64   2  32  buffered_future_mask (-inf above j = i)  yes
  m2    k is v         130  67   2  128  2  64  mixed (finite values with -inf holes)    yes
  m3    three tensors  5    5    2  50   2  25  None                                     no
  m4    k is v         65   67   2  192  2  96  finite                                   yes
"""
import numpy as np

from detgen import det

# tag, call form, T, S, B, d, H, mask kind, bias
CASES = (("m1", "qkv", 65, 65, 3, 64, 2, "future", True),
         ("m2", "kv", 130, 67, 2, 128, 2, "mixed", True),
         ("m3", "sep", 5, 5, 2, 50, 2, None, False),
         ("m4", "kv", 65, 67, 2, 192, 2, "finite", True))
THIN_ABOVE = 16384      # tensors with more elements are stored as every fourth slice (and the last) of one dimension


def make_mask(kind, T, S, pfx):
    """float32 [T, S] (or None); every row keeps a visible key by construction."""
    if kind is None:
        return None
    ninf = np.float32(-np.inf)
    if kind == "future":            # what buffered_future_mask(query, key) returns: -inf where j - i >= 1 + |S - T|
        j, i = np.meshgrid(np.arange(S), np.arange(T))
        return np.where(j - i >= 1 + abs(S - T), ninf, np.float32(0)).astype(np.float32)
    finite = det(pfx + "mask.f", (T, S), 2.0)
    if kind == "finite":
        return finite
    hidden = det(pfx + "mask.u", (T, S)) > 0.2533          # P(N(0,1) > 0.2533) = 0.4
    rows = np.arange(T)
    hidden[rows, rows % S] = False
    if S > 64:                      # odd rows: the whole first 64-key tile hidden, key 64 visible
        hidden[1::2, :64] = True
        hidden[1::2, 64] = False
    dead = S // 3                   # one key no query sees
    hidden[:, dead] = True
    for i in range(T):
        if hidden[i].all():
            hidden[i, (dead + 1) % S] = False
    assert (~hidden).any(axis=1).all()
    return np.where(hidden, ninf, finite).astype(np.float32)


def thin(name, a):
    """(index array or None, the stored part of `a`): the head-averaged weights [B, T, S] are thinned over T, every other
    tensor over its first dimension."""
    if a.size <= THIN_ABOVE:
        return None, a
    dim = 1 if name == "weights" else 0
    n = a.shape[dim]
    idx = np.array(sorted(set(range(0, n, 4)) | {n - 1}))
    return idx, np.take(a, idx, axis=dim)
