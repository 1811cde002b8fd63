"""No-GPU checks of key_padding_mask: the ctypes signatures of the six new entries, host-side argument validation (nothing
is launched: every call made here is one the library must reject, with made-up addresses), the ops wrappers, the module's
refusals, and the fp64 restatement of tests/mha_kpm_cases.py against the reference's own sample-by-sample run
(tests/golden/mha_kpm.npz).

The restatement's limit against the fixture is 2e-6 * max(1, |ref|max), the limit tests/test_mha_bias_cpu.py uses for the
same comparison: the fixture is the reference's fp32 run, whose own rounding is what separates the two (measured: at most
5.4e-7 on k1 - k3)."""
import ctypes as C
import os
import re

import numpy as np
import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, ops
from bpmult_amd.models import MultiheadAttention
from mha_kpm_cases import CASES, REFERENCE_RUNS, case, learned_bias, padding, restate, visible

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bpmult_hip.h")).read()
G = dict(np.load(os.path.join(ROOT, "tests", "golden", "mha_kpm.npz")))
ERR_ARG = -1
NEW = ("bpm_attn_maps_kmask", "bpm_attn_fwd_kamask", "bpm_attn_bwd_dq_kamask", "bpm_attn_bwd_dkv_kamask", "bpm_attn_maps_kamask",
       "bpm_attn_bwd_dbias_kmask")


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def test_signatures_exist_and_the_abi_version_is_still_5(lib):
    assert lib.bpm_version() == 5 and _lib.ABI_VERSION == 5
    assert int(re.search(r"#define BPM_ABI_VERSION (\d+)", HEADER).group(1)) == 5
    for name in NEW:
        assert name in _lib.SIGNATURES and re.search(rf"\bint {name}\(", HEADER), name
        assert C.POINTER(_lib.AttnKMask) in _lib.SIGNATURES[name], name
        assert callable(getattr(lib, name)), name
    for name in NEW[1:]:
        assert C.POINTER(_lib.AttnHMask) in _lib.SIGNATURES[name], name
    assert _lib.SIGNATURES["bpm_attn_bwd_dbias_ws_bytes"] == [C.POINTER(_lib.AttnProblem), C.POINTER(_lib.AttnDBias), _lib._I], "unchanged"
    for fn in ("attn_maps_kmask", "attn_fwd_kamask", "attn_bwd_dq_kamask", "attn_bwd_dkv_kamask", "attn_maps_kamask"):
        assert callable(getattr(ops, fn)), fn


# --- argument validation -------------------------------------------------------------------------------------------------
T_, S_ = 9, 10
WS, WS_BYTES = 0x400000, 1 << 20


def _problem(**kw):
    a = _lib.AttnProblem()
    a.Q, a.K, a.V, a.O, a.lse, a.dO, a.delta, a.dQ, a.dK, a.dV = (0x10000 * (i + 1) for i in range(10))
    a.ldo = a.lddq = a.lddk = a.lddv = 64
    a.B, a.H, a.T, a.S, a.dh, a.dhp = 4, 2, T_, S_, 32, 32
    a.dq_scale = 1.0
    for n, v in kw.items():
        setattr(a, n, v)
    return a


def _map_problem(**kw):
    m = _lib.AttnMapProblem()
    m.Q, m.K, m.lse, m.W, m.ldw = 0x10000, 0x20000, 0x30000, 0x40000, S_
    m.B, m.H, m.T, m.S, m.dh, m.dhp = 4, 2, T_, S_, 32, 32
    for n, v in kw.items():
        setattr(m, n, v)
    return m


def _kmask(**kw):
    k = _lib.AttnKMask()
    k.mask, k.ldm = 0x500000, S_
    for n, v in kw.items():
        setattr(k, n, v)
    return k


def _amask(**kw):
    k = _lib.AttnHMask()
    k.mask, k.ldm, k.maskT, k.ldt = 0x100000, 12, 0x200000, 12
    for n, v in kw.items():
        setattr(k, n, v)
    return k


def _out():
    o = _lib.AttnDBias()
    o.dB, o.lddb, o.head_stride = 0x300000, 12, 0
    return o


def _ref(x):
    return None if x is None else C.byref(x)


def _calls(lib, which, prob=None, mp=None, km="default", am="default", n=1, dtype=_lib.BPM_F32):
    """The entries named in `which`, each called once with the same (bad) arguments -> {name: return code}."""
    prob = _problem() if prob is None else prob
    mp = _map_problem() if mp is None else mp
    km = _kmask() if km == "default" else km
    am = _amask() if am == "default" else am
    o = _out()
    out = {}
    for w in which:
        if w == "maps_kmask":
            out[w] = lib.bpm_attn_maps_kmask(dtype, C.byref(mp), _ref(km), n, None)
        elif w == "maps_kamask":
            out[w] = lib.bpm_attn_maps_kamask(dtype, C.byref(mp), _ref(km), _ref(am), n, None)
        elif w == "dbias_kmask":
            out[w] = lib.bpm_attn_bwd_dbias_kmask(dtype, C.byref(prob), _ref(am), _ref(km), C.byref(o), n, 0, WS, WS_BYTES, None)
        else:
            out[w] = getattr(lib, f"bpm_attn_{w}_kamask")(dtype, C.byref(prob), _ref(km), _ref(am), n, 0, None)
    return out


ATTN = ("fwd", "bwd_dq", "bwd_dkv")
BYTE_READERS = ATTN + ("maps_kmask", "maps_kamask", "dbias_kmask")
IMAGE_READERS = ATTN + ("maps_kamask", "dbias_kmask")
TRANSPOSE_READERS = ("bwd_dkv", "maps_kamask")
# what, the entries that read the argument, the bad arguments.  (A NULL kmasks ARRAY is legal for bpm_attn_bwd_dbias_kmask: it
# is bpm_attn_bwd_dbias then; that call is not made here.)
BAD = [("no byte-mask array", ATTN + ("maps_kmask", "maps_kamask"), dict(km=None)),
       ("no additive-mask array", IMAGE_READERS, dict(am=None)),
       ("NULL byte mask", BYTE_READERS, dict(km=_kmask(mask=None))),
       ("byte ldm < S", BYTE_READERS, dict(km=_kmask(ldm=S_ - 1))),
       ("NULL additive mask", IMAGE_READERS, dict(am=_amask(mask=None))),
       ("additive ldm < S", IMAGE_READERS, dict(am=_amask(ldm=8))),
       ("additive ldm % 4", IMAGE_READERS, dict(am=_amask(ldm=11))),
       ("additive mask not 16-byte aligned", IMAGE_READERS, dict(am=_amask(mask=0x100004))),
       ("head_stride < T * ldm", IMAGE_READERS, dict(am=_amask(head_stride=T_ * 12 - 4, head_strideT=S_ * 12))),
       ("head_stride % 4", IMAGE_READERS, dict(am=_amask(head_stride=T_ * 12 + 2, head_strideT=S_ * 12))),
       ("NULL maskT", TRANSPOSE_READERS, dict(am=_amask(maskT=None))),
       ("ldt < T", TRANSPOSE_READERS, dict(am=_amask(ldt=8))),
       ("ldt % 4", TRANSPOSE_READERS, dict(am=_amask(ldt=10))),
       ("maskT not 16-byte aligned", TRANSPOSE_READERS, dict(am=_amask(maskT=0x200008))),
       ("head_strideT < S * ldt", TRANSPOSE_READERS, dict(am=_amask(head_stride=T_ * 12, head_strideT=S_ * 12 - 4))),
       ("dS / Pd set", ATTN + ("dbias_kmask",),
        dict(prob=_problem(S=12, dS=0x600000, Pd=0x700000, xs_b=4096, xs_h=1024, xs_q=12), km=_kmask(ldm=12))),
       ("nprob 0", BYTE_READERS, dict(n=0)),
       ("more problems than a launch takes", BYTE_READERS, dict(n=_lib.MAX_GROUP + 1)),
       ("unknown dtype", BYTE_READERS, dict(dtype=2)),
       ("dhp no kernel has", BYTE_READERS, dict(prob=_problem(dhp=48, dh=40), mp=_map_problem(dhp=48, dh=40)))]


@pytest.mark.parametrize("what,which,bad", BAD, ids=[b[0] for b in BAD])
def test_every_entry_that_reads_an_argument_rejects_a_bad_one(lib, what, which, bad):
    assert _calls(lib, which, **bad) == {w: ERR_ARG for w in which}, what


def test_mixed_dhp_in_one_launch_is_refused(lib):
    probs = (_lib.AttnProblem * 2)(_problem(), _problem(dhp=64, dh=64))
    mps = (_lib.AttnMapProblem * 2)(_map_problem(), _map_problem(dhp=64, dh=64))
    kms = (_lib.AttnKMask * 2)(_kmask(), _kmask())
    ams = (_lib.AttnHMask * 2)(_amask(), _amask())
    outs = (_lib.AttnDBias * 2)(_out(), _out())
    for name in ("bpm_attn_fwd_kamask", "bpm_attn_bwd_dq_kamask", "bpm_attn_bwd_dkv_kamask"):
        assert getattr(lib, name)(_lib.BPM_BF16, probs, kms, ams, 2, 0, None) == ERR_ARG, name
    assert lib.bpm_attn_maps_kmask(_lib.BPM_BF16, mps, kms, 2, None) == ERR_ARG
    assert lib.bpm_attn_maps_kamask(_lib.BPM_BF16, mps, kms, ams, 2, None) == ERR_ARG
    assert lib.bpm_attn_bwd_dbias_kmask(_lib.BPM_BF16, probs, ams, kms, outs, 2, 0, WS, WS_BYTES, None) == ERR_ARG


def test_the_second_problem_of_a_launch_is_checked_too(lib):
    probs = (_lib.AttnProblem * 2)(_problem(), _problem())
    ams = (_lib.AttnHMask * 2)(_amask(), _amask())
    kms = (_lib.AttnKMask * 2)(_kmask(), _kmask(ldm=S_ - 1))
    assert lib.bpm_attn_fwd_kamask(_lib.BPM_F32, probs, kms, ams, 2, 0, None) == ERR_ARG
    kms = (_lib.AttnKMask * 2)(_kmask(), _kmask())
    ams = (_lib.AttnHMask * 2)(_amask(), _amask(ldm=11))
    assert lib.bpm_attn_bwd_dq_kamask(_lib.BPM_F32, probs, kms, ams, 2, 0, None) == ERR_ARG


def test_workspace_rules_of_the_bias_gradient_hold_with_byte_masks(lib):
    prob, am, km, o = _problem(), _amask(), _kmask(), _out()
    need = lib.bpm_attn_bwd_dbias_ws_bytes(C.byref(prob), C.byref(o), 1)
    assert 16 < need <= WS_BYTES, "the made-up call above splits its heads: the workspace rules below are real refusals"
    for ws, nbytes in ((None, WS_BYTES), (WS, 16), (WS + 4, WS_BYTES)):
        assert lib.bpm_attn_bwd_dbias_kmask(_lib.BPM_F32, C.byref(prob), C.byref(am), C.byref(km), C.byref(o), 1, 0, ws, nbytes, None) == ERR_ARG


# --- ops wrappers ------------------------------------------------------------------------------------------------------------
def test_ops_wrappers_raise_before_calling(monkeypatch):
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.attn_kmasks([(torch.zeros(2, 10, dtype=torch.uint8), 10)])
    monkeypatch.setattr(ops, "_DRY_RUN", True)            # host tensors stand in for device pointers; nothing is launched
    monkeypatch.setattr(ops, "_DRY_LAUNCHES", [])
    km = ops.attn_kmasks([(torch.ones(4, S_, dtype=torch.uint8), S_)])
    am = ops.attn_amasks([(torch.zeros(T_, 12), 12, torch.zeros(S_, 12), 12)])
    none_k, none_a = ops.attn_kmasks([]), ops.attn_amasks([])
    for fn in (ops.attn_fwd_kamask, ops.attn_bwd_dq_kamask, ops.attn_bwd_dkv_kamask):
        with pytest.raises(ValueError, match="one key mask and one additive mask per problem"):
            fn(_lib.BPM_F32, [_problem()], none_k, am)
        with pytest.raises(ValueError, match="one key mask and one additive mask per problem"):
            fn(_lib.BPM_F32, [_problem()], km, none_a)
    with pytest.raises(ValueError, match="one key mask and one additive mask per problem"):
        ops.attn_maps_kamask(_lib.BPM_F32, [_map_problem()], km, none_a)
    with pytest.raises(ValueError, match="one key mask per problem"):
        ops.attn_maps_kmask(_lib.BPM_F32, [_map_problem()], none_k)
    g = ops.attn_dbias([(torch.zeros(T_, 12), 12, 0)])
    with pytest.raises(ValueError, match="one key mask per problem"):
        ops.attn_bwd_dbias(_lib.BPM_F32, [_problem()], am, g, kmasks=none_k)
    with pytest.raises(ValueError, match="expected uint8"):
        ops.attn_kmasks([(torch.ones(4, S_, dtype=torch.bool), S_)])
    # the maps wrappers record under _DRY_RUN, as attn_maps does
    ops.attn_maps_kmask(_lib.BPM_F32, [_map_problem()], km)
    ops.attn_maps_kamask(_lib.BPM_F32, [_map_problem()], km, am)
    assert [rec[0] for rec in ops._DRY_LAUNCHES] == [ops.attn_maps_kmask, ops.attn_maps_kamask]


# --- the module --------------------------------------------------------------------------------------------------------------
def test_module_refusals():
    m = MultiheadAttention(24, 4)
    x, y = torch.zeros(3, 2, 24), torch.zeros(5, 2, 24)            # T = 3, S = 5, B = 2
    ok = torch.zeros(2, 5, dtype=torch.bool)
    with pytest.raises(ValueError, match=r"key_padding_mask of shape \(2, 6\), expected \[2, 5\]"):
        m(x, y, y, key_padding_mask=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="key_padding_mask of shape"):
        m(x, y, y, key_padding_mask=torch.zeros(5, 2, dtype=torch.uint8))      # [S, B]
    with pytest.raises(ValueError, match="key_padding_mask must be a torch.bool or torch.uint8 tensor"):
        m(x, y, y, key_padding_mask=torch.zeros(2, 5))
    with pytest.raises(ValueError, match="key_padding_mask must be"):
        m(x, y, y, key_padding_mask=torch.zeros(2, 5, dtype=torch.int64))
    with pytest.raises(ValueError, match="key_padding_mask must be"):
        m(x, y, y, key_padding_mask=[[0] * 5] * 2)
    with pytest.raises(ValueError, match="key_padding_mask must be"):      # only a float tensor can ask for a gradient
        m(x, y, y, key_padding_mask=torch.zeros(2, 5, requires_grad=True))
    with pytest.raises(ValueError, match="key_padding_mask on meta, the inputs on cpu"):
        m(x, y, y, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool, device="meta"))
    m.precision = "bf16x3"
    with pytest.raises(ValueError, match="bf16x3"):
        m(x, y, y, key_padding_mask=ok)
    m.precision = None
    with pytest.raises(ValueError, match="no gradient"):              # attn_mask keeps its refusal beside a padding mask
        m(x, y, y, attn_mask=torch.zeros(3, 5, requires_grad=True), key_padding_mask=ok)
    for flag in ("add_bias_kv", "add_zero_attn"):
        with pytest.raises(ValueError, match=flag):
            MultiheadAttention(24, 4, **{flag: True})
    # valid arguments: only the device is missing
    for kw in (dict(key_padding_mask=ok), dict(key_padding_mask=ok.to(torch.uint8), attn_mask=torch.zeros(3, 5)),
               dict(key_padding_mask=ok, attn_bias=torch.zeros(4, 3, 5, requires_grad=True), need_weights=False)):
        with pytest.raises(RuntimeError, match="no CPU path"):
            m(x, y, y, **kw)


# --- the restatement against the reference's run -----------------------------------------------------------------------------
def test_the_fixture_holds_the_reference_runs():
    assert sorted({k.split(".")[0] for k in G}) == sorted(REFERENCE_RUNS)
    assert [c[0] for c in CASES] == ["k1", "k2", "k3", "k4"]


@pytest.mark.parametrize("tag", REFERENCE_RUNS)
def test_restatement_reproduces_the_reference(tag):
    c = case(tag)
    got = restate(c)
    names = sorted(k[len(tag) + 1:] for k in G if k.startswith(tag + ".") and not k.endswith((".idx", ".n")))
    assert sorted(got) == names, (sorted(got), names)
    for name in names:
        key = f"{tag}.{name}"
        a = got[name].numpy()
        assert np.isfinite(a).all(), key
        ref, idx, (rn, rs) = G[key], G.get(key + ".idx"), G[key + ".n"]
        assert abs(np.linalg.norm(a.ravel()) - rn) <= 2e-6 * max(1.0, rn), key
        if idx is not None:
            a = np.take(a, idx, axis=1 if name == "weights" else 0)
        assert a.shape == ref.shape, (key, a.shape, ref.shape)
        scale = max(1.0, float(np.abs(ref).max()))
        err = float(np.abs(a - ref).max())
        print(f"{key}: max err {err:.3e} (scale {scale:.3g})")
        assert err <= 2e-6 * scale, f"{key}: {err:.3e} > {2e-6 * scale:.3e}"


@pytest.mark.parametrize("tag", [c[0] for c in CASES])
def test_restatement_hides_what_the_masks_hide(tag):
    c = case(tag)
    got = restate(c)
    pm = padding(c)                                                           # [B, S]
    w = got["weights"].numpy()                                                # [B, T, S]
    assert (w[np.broadcast_to(pm[:, None, :], w.shape)] == 0).all(), "a padded key has weight exactly 0"
    assert np.abs(w.sum(-1) - 1).max() <= 1e-12
    if "gk" in got:
        gk = got["gk"].numpy()                                                # [S, B, d]
        if "gv" in got or c[1] == "kv":
            assert (gk[pm.T] == 0).all(), "d(key) of a padded position is exactly 0 (k is v: d(key) + d(value))"
    if "gv" in got:
        assert (got["gv"].numpy()[pm.T] == 0).all()
    if learned_bias(c) is not None:
        g = got["g.bias"].numpy()
        g = g if g.ndim == 3 else g[None]
        never = ~visible(c).any(0)                                            # [Hm, T, S]: hidden in every sample
        assert (g[never] == 0).all(), "no sample contributes at a pair hidden in all of them"
        assert np.abs(g.sum(-1)).max() <= 1e-12, "softmax backward: the rows of the score gradient sum to 0"
