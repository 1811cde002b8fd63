"""No-GPU checks of the learned attention bias: the fp64 restatement of tests/mha_bias_cases.py against the reference's own
run (tests/golden/mha_bias.npz), host-side argument validation of bpm_attn_bwd_dbias (nothing is launched: every call made
here is one the library must reject), the head stride of bpm_attn_hmask, the workspace query and the module's refusals.

The restatement's limit against the fixture is 2e-6 * max(1, |ref|max): the fixture is the reference's fp32 run, whose own
rounding is what separates the two (measured against the reference run directly: 2.3e-7 - 3.1e-7)."""
import ctypes as C
import os

import numpy as np
import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, ops
from bpmult_amd.models import MultiheadAttention
from mha_bias_cases import CASES, case, head_bias, restate, shared_bias

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
G = dict(np.load(os.path.join(ROOT, "tests", "golden", "mha_bias.npz")))
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_restatement_reproduces_the_reference(tag):
    c = case(tag)
    bias = shared_bias(c)
    got = restate(c, bias)
    names = sorted(k[len(tag) + 1:] for k in G if k.startswith(tag + ".") and not k.endswith((".idx", ".n")))
    assert sorted(got) == names, (sorted(got), names)
    for name in names:
        key = f"{tag}.{name}"
        a = got[name].numpy()
        ref, idx, (rn, rs) = G[key], G.get(key + ".idx"), G[key + ".n"]
        assert abs(np.linalg.norm(a.ravel()) - rn) <= 2e-6 * max(1.0, rn), key
        if idx is not None:
            a = np.take(a, idx, axis=1 if name == "weights" else 0)
        assert a.shape == ref.shape, (key, a.shape, ref.shape)
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(a - ref).max())
        print(f"{key}: max err {err:.3e} (scale {scale:.3g})")
        assert err <= 2e-6 * scale, f"{key}: {err:.3e} > {2e-6 * scale:.3e}"
    g = got["g.bias"].numpy()
    assert (g[np.isinf(bias)] == 0).all(), "the gradient of a -inf entry is exactly 0"
    assert np.abs(g.sum(-1)).max() <= 1e-12, "softmax backward: the rows of the score gradient sum to 0"


@pytest.mark.parametrize("tag", ["b1", "b2"])
def test_per_head_gradient_of_a_repeated_image_sums_to_the_shared_gradient(tag):
    c = case(tag)
    bias = shared_bias(c)
    shared = restate(c, bias)
    heads = restate(c, np.stack([bias] * c[6]))
    assert heads["g.bias"].shape == (c[6],) + bias.shape
    assert float((heads["g.bias"].sum(0) - shared["g.bias"]).abs().max()) <= 1e-12
    for n in shared:
        if n != "g.bias":
            assert float((heads[n] - shared[n]).abs().max()) <= 1e-12, n
    other = restate(c, head_bias(c))
    assert float((other["attn"] - shared["attn"]).abs().max()) > 1e-3, "different images per head must change the output"


# --- bpm_attn_bwd_dbias: argument validation (made-up 16-byte aligned addresses: only rejected calls are made) -----------
T_, S_ = 9, 10


def _problem(**kw):
    a = _lib.AttnProblem()
    a.Q, a.K, a.V, a.O, a.lse, a.dO, a.delta, a.dQ, a.dK, a.dV = (0x10000 * (i + 1) for i in range(10))
    a.ldo = a.lddq = a.lddk = a.lddv = 64
    a.B, a.H, a.T, a.S, a.dh, a.dhp = 4, 2, T_, S_, 32, 32
    a.dq_scale = 1.0
    for n, v in kw.items():
        setattr(a, n, v)
    return a


def _mask(**kw):
    k = _lib.AttnHMask()
    k.mask, k.ldm, k.maskT, k.ldt = 0x100000, 12, 0x200000, 12
    for n, v in kw.items():
        setattr(k, n, v)
    return k


def _out(**kw):
    o = _lib.AttnDBias()
    o.dB, o.lddb, o.head_stride = 0x300000, 12, 0
    for n, v in kw.items():
        setattr(o, n, v)
    return o


WS, WS_BYTES = 0x400000, 1 << 20


def _call(lib, prob, k, o, ws=WS, ws_bytes=WS_BYTES, n=1, dtype=_lib.BPM_F32):
    ref = lambda x: None if x is None else C.byref(x)
    return lib.bpm_attn_bwd_dbias(dtype, ref(prob), ref(k), ref(o), n, 0, ws, ws_bytes, None)


BAD = [("no problems", dict(prob=None)), ("no masks", dict(k=None)), ("no outputs", dict(o=None)),
       ("nprob 0", dict(n=0)), ("unknown dtype", dict(dtype=2)),
       ("NULL Q", dict(prob=_problem(Q=None))), ("NULL dO", dict(prob=_problem(dO=None))), ("NULL delta", dict(prob=_problem(delta=None))),
       ("NULL lse", dict(prob=_problem(lse=None))), ("NULL mask", dict(k=_mask(mask=None))), ("NULL dB", dict(o=_out(dB=None))),
       ("lddb < S", dict(o=_out(lddb=8))), ("lddb % 4", dict(o=_out(lddb=11))), ("dB not 16-byte aligned", dict(o=_out(dB=0x300004))),
       ("head_stride < T * lddb", dict(o=_out(head_stride=T_ * 12 - 4))), ("head_stride % 4", dict(o=_out(head_stride=T_ * 12 + 2))),
       ("mask head_stride < T * ldm", dict(k=_mask(head_stride=T_ * 12 - 4))), ("mask head_stride % 4", dict(k=_mask(head_stride=T_ * 12 + 1))),
       ("ldm < S", dict(k=_mask(ldm=8))), ("mask not 16-byte aligned", dict(k=_mask(mask=0x100004))),
       ("no workspace", dict(ws=None)), ("short workspace", dict(ws_bytes=16)), ("workspace not 16-byte aligned", dict(ws=WS + 4)),
       ("dS / Pd set", dict(prob=_problem(S=12, dS=0x500000, Pd=0x600000, xs_b=4096, xs_h=1024, xs_q=12), o=_out(lddb=12))),
       ("dhp no kernel has", dict(prob=_problem(dhp=48, dh=40)))]


@pytest.mark.parametrize("what,bad", BAD, ids=[b[0] for b in BAD])
def test_dbias_entry_rejects_bad_arguments_before_a_launch(lib, what, bad):
    args = dict(prob=_problem(), k=_mask(), o=_out())
    args.update(bad)
    assert _call(lib, args.pop("prob"), args.pop("k"), args.pop("o"), **args) == ERR_ARG, what


def test_the_valid_call_of_the_table_above_needs_a_workspace(lib):
    """The cases above differ from one valid call in one argument each: that call's head range is split (B * H = 8 heads,
    one tile), so `no workspace` and `short workspace` are real refusals and not side effects."""
    prob, o = _problem(), _out()
    need = lib.bpm_attn_bwd_dbias_ws_bytes(C.byref(prob), C.byref(o), 1)
    assert need == 2 * T_ * 12 * 4 and 16 < need <= WS_BYTES       # two splits of four heads, one [T, ldp] image each
    prob = _problem(B=4, H=1)
    o = _out(head_stride=T_ * 12)                 # per head: 4 samples feed the one image -> one workgroup of DB_MIN_TERMS heads
    assert lib.bpm_attn_bwd_dbias_ws_bytes(C.byref(prob), C.byref(o), 1) == 0


def test_mixed_dhp_in_one_launch_is_refused(lib):
    probs = (_lib.AttnProblem * 2)(_problem(), _problem(dhp=64, dh=64))
    masks = (_lib.AttnHMask * 2)(_mask(), _mask())
    outs = (_lib.AttnDBias * 2)(_out(), _out(dB=0x700000))
    assert lib.bpm_attn_bwd_dbias(_lib.BPM_BF16, probs, masks, outs, 2, 0, WS, WS_BYTES, None) == ERR_ARG
    assert lib.bpm_attn_bwd_dbias_ws_bytes(probs, outs, 2) == 0
    assert lib.bpm_attn_bwd_dbias(_lib.BPM_BF16, probs, masks, outs, _lib.MAX_GROUP + 1, 0, WS, WS_BYTES, None) == ERR_ARG


def test_a_bad_head_stride_is_refused_by_the_mask_entries_too(lib):
    prob, mp = _problem(), _lib.AttnMapProblem()
    mp.Q, mp.K, mp.lse, mp.W, mp.ldw = 0x10000, 0x20000, 0x30000, 0x40000, S_
    mp.B, mp.H, mp.T, mp.S, mp.dh, mp.dhp = 2, 2, T_, S_, 32, 32
    for bad in (dict(head_stride=T_ * 12 - 4), dict(head_stride=T_ * 12 + 2), dict(head_stride=1 << 31)):
        k = _mask(**bad)
        assert lib.bpm_attn_fwd_hmask(_lib.BPM_F32, C.byref(prob), C.byref(k), 1, 0, None) == ERR_ARG, bad
        assert lib.bpm_attn_bwd_dq_hmask(_lib.BPM_F32, C.byref(prob), C.byref(k), 1, 0, None) == ERR_ARG, bad
    for bad in (dict(head_strideT=S_ * 12 - 4), dict(head_strideT=S_ * 12 + 2), dict(head_stride=T_ * 12 - 4, head_strideT=S_ * 12)):
        k = _mask(**bad)
        assert lib.bpm_attn_bwd_dkv_hmask(_lib.BPM_F32, C.byref(prob), C.byref(k), 1, 0, None) == ERR_ARG, bad
        assert lib.bpm_attn_maps_hmask(_lib.BPM_F32, C.byref(mp), C.byref(k), 1, None) == ERR_ARG, bad


def test_ctypes_mirror_of_the_new_structs():
    assert [f[0] for f in _lib.AttnDBias._fields_] == ["dB", "lddb", "head_stride"] and C.sizeof(_lib.AttnDBias) == 24
    assert [f[0] for f in _lib.AttnHMask._fields_] == [f[0] for f in _lib.AttnAMask._fields_] + ["head_stride", "head_strideT"]
    assert C.sizeof(_lib.AttnHMask) == 48 and C.sizeof(_lib.AttnAMask) == 32, "bpm_attn_amask and its entries are unchanged"
    for name in ("bpm_attn_fwd_hmask", "bpm_attn_bwd_dq_hmask", "bpm_attn_bwd_dkv_hmask", "bpm_attn_maps_hmask", "bpm_attn_bwd_dbias"):
        assert C.POINTER(_lib.AttnHMask) in _lib.SIGNATURES[name], name
    assert _lib.PROF_KINDS["attn_bwd_dbias"] == 17


def test_ops_wrappers(monkeypatch):
    monkeypatch.setattr(ops, "_DRY_RUN", True)            # host tensors stand in for device pointers; nothing is launched
    m, mt = torch.zeros(2, 9, 12), torch.zeros(2, 10, 12)
    (a,) = ops.attn_amasks([(m[0], 12, mt[0], 12)])
    assert (a.head_stride, a.head_strideT, a.ldm, a.ldt) == (0, 0, 12, 12), "a 4-tuple is one image for all heads"
    (b,) = ops.attn_amasks([(m, 12, mt, 12, 9 * 12, 10 * 12)])
    assert (b.head_stride, b.head_strideT, b.mask, b.maskT) == (108, 120, m.data_ptr(), mt.data_ptr())
    g = torch.zeros(9, 12)
    (o,) = ops.attn_dbias([(g, 12, 0)])
    assert (o.dB, o.lddb, o.head_stride) == (g.data_ptr(), 12, 0)
    with pytest.raises(ValueError, match="expected float32"):
        ops.attn_dbias([(g.double(), 12, 0)])
    with pytest.raises(ValueError, match="one mask and one output per problem"):
        ops.attn_bwd_dbias(_lib.BPM_F32, [_problem()], ops.attn_amasks([]), ops.attn_dbias([(g, 12, 0)]))
    with pytest.raises(ValueError, match="one output per problem"):
        ops.attn_dbias_ws_bytes([_problem()], ops.attn_dbias([]))


def test_ops_wrappers_have_no_cpu_fallback():
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.attn_dbias([(torch.zeros(9, 12), 12, 0)])


def test_workspace_query_is_monotone_in_the_heads_of_the_shared_form(lib):
    o = _out()
    sizes = []
    for B, H in ((1, 1), (1, 2), (2, 2), (3, 2), (4, 2), (3, 4), (9, 4), (8, 12), (64, 12)):
        prob = _problem(B=B, H=H)
        sizes.append(ops.attn_dbias_ws_bytes([prob], (_lib.AttnDBias * 1)(o)))
    assert sizes == sorted(sizes) and sizes[0] == 0 and sizes[-1] > sizes[3] > 0, sizes
    # the split stops at the chip (256 compute units x 3 resident workgroups at head_dim 64): the attention shape of
    # DESIGN.md section 5 has 64 tiles and gets 12 workgroups per tile
    prob = _problem(B=8, H=12, T=512, S=512, dh=64, dhp=64)
    shared = ops.attn_dbias_ws_bytes([prob], (_lib.AttnDBias * 1)(_out(lddb=512)))
    assert shared == 12 * 512 * 512 * 4
    assert ops.attn_dbias_ws_bytes([prob], (_lib.AttnDBias * 1)(_out(lddb=512, head_stride=512 * 512))) == 0, "768 tiles: no split"


def test_module_refusals():
    m = MultiheadAttention(24, 4)
    x = torch.zeros(3, 2, 24)
    with pytest.raises(ValueError, match=r"attn_bias of shape \(3, 4\)"):
        m(x, x, x, attn_bias=torch.zeros(3, 4))
    with pytest.raises(ValueError, match="attn_bias of shape"):
        m(x, x, x, attn_bias=torch.zeros(2, 3, 3))                  # 2 is the batch, not the heads
    with pytest.raises(ValueError, match="attn_bias of shape"):
        m(x, x, x, attn_bias=torch.zeros(2, 4, 3, 3))
    with pytest.raises(ValueError, match="float32"):
        m(x, x, x, attn_bias=torch.zeros(3, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="float32"):
        m(x, x, x, attn_bias=[[0.0] * 3] * 3)
    with pytest.raises(ValueError, match="the inputs on"):
        m(x, x, x, attn_bias=torch.zeros(3, 3, device="meta"))
    m.precision = "bf16x3"
    with pytest.raises(ValueError, match="bf16x3"):
        m(x, x, x, attn_bias=torch.zeros(4, 3, 3))
    m.precision = None
    with pytest.raises(ValueError, match="no gradient"):            # attn_mask keeps its refusal beside a bias
        m(x, x, x, attn_mask=torch.zeros(3, 3, requires_grad=True), attn_bias=torch.zeros(3, 3))
    with pytest.raises(RuntimeError, match="no CPU path"):          # valid arguments: only the device is missing
        m(x, x, x, attn_bias=torch.zeros(4, 3, 3, requires_grad=True))
