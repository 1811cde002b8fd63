"""No-GPU checks of the additive-mask attention entries and the MultiheadAttention module: the ctypes mirror of
bpm_attn_amask, host-side argument validation of the four *_amask entries (nothing is launched: every call made here is
one the library must reject), the module's state_dict layout and constructor / input refusals."""
import ctypes as C
import os
import re

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, ops
from bpmult_amd.models import MultiheadAttention

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bpmult_hip.h")).read()
ERR_ARG = -1


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def test_abi_version_is_still_5(lib):
    assert lib.bpm_version() == 5 and _lib.ABI_VERSION == 5
    assert int(re.search(r"#define BPM_ABI_VERSION (\d+)", HEADER).group(1)) == 5


def test_ctypes_struct_mirrors_the_header():
    body = re.search(r"typedef struct bpm_attn_amask \{(.*?)\} bpm_attn_amask;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    decls = [d.strip() for d in body.split(";") if d.strip()]
    names = [d.split()[-1].lstrip("*") for d in decls]
    assert names == [f[0] for f in _lib.AttnAMask._fields_] == ["mask", "ldm", "maskT", "ldt"]
    kinds = ["ptr" if "*" in d else "int" for d in decls]
    assert kinds == ["ptr" if f[1] is C.c_void_p else "int" for f in _lib.AttnAMask._fields_]
    assert C.sizeof(_lib.AttnAMask) == 32
    for name in ("bpm_attn_fwd_amask", "bpm_attn_bwd_dq_amask", "bpm_attn_bwd_dkv_amask", "bpm_attn_maps_amask"):
        assert C.POINTER(_lib.AttnAMask) in _lib.SIGNATURES[name], name
    for fn in ("attn_amasks", "attn_fwd_amask", "attn_bwd_dq_amask", "attn_bwd_dkv_amask", "attn_maps_amask"):
        assert callable(getattr(ops, fn)), fn


T_, S_ = 9, 10          # made-up 16-byte aligned addresses below: only rejected calls are made, nothing is dereferenced


def _problem():
    a = _lib.AttnProblem()
    a.Q, a.K, a.V, a.O, a.lse, a.dO, a.delta, a.dQ, a.dK, a.dV = (0x10000 * (i + 1) for i in range(10))
    a.ldo = a.lddq = a.lddk = a.lddv = 64
    a.B, a.H, a.T, a.S, a.dh, a.dhp = 2, 2, T_, S_, 32, 32
    a.dq_scale = 1.0
    return a


def _map_problem():
    m = _lib.AttnMapProblem()
    m.Q, m.K, m.lse, m.W, m.ldw = 0x10000, 0x20000, 0x30000, 0x40000, S_
    m.B, m.H, m.T, m.S, m.dh, m.dhp = 2, 2, T_, S_, 32, 32
    return m


def _mask(**kw):
    k = _lib.AttnAMask()
    k.mask, k.ldm, k.maskT, k.ldt = 0x100000, 12, 0x200000, 12
    for n, v in kw.items():
        setattr(k, n, v)
    return k


def _calls(lib, prob, mp, k):
    kp = None if k is None else C.byref(k)
    return {"fwd": lib.bpm_attn_fwd_amask(_lib.BPM_F32, C.byref(prob), kp, 1, 0, None),
            "dq": lib.bpm_attn_bwd_dq_amask(_lib.BPM_BF16, C.byref(prob), kp, 1, 0, None),
            "dkv": lib.bpm_attn_bwd_dkv_amask(_lib.BPM_F32, C.byref(prob), kp, 1, 0, None),
            "maps": lib.bpm_attn_maps_amask(_lib.BPM_BF16, C.byref(mp), kp, 1, None)}


@pytest.mark.parametrize("what,bad", [("no mask array", None), ("NULL mask", dict(mask=None)), ("ldm < S", dict(ldm=8)),
                                      ("ldm % 4", dict(ldm=11)), ("mask not 16-byte aligned", dict(mask=0x100004))])
def test_all_four_entries_reject_a_bad_mask(lib, what, bad):
    k = None if bad is None else _mask(**bad)
    assert _calls(lib, _problem(), _map_problem(), k) == {"fwd": ERR_ARG, "dq": ERR_ARG, "dkv": ERR_ARG, "maps": ERR_ARG}, what


@pytest.mark.parametrize("what,bad", [("NULL maskT", dict(maskT=None)), ("ldt < T", dict(ldt=8)), ("ldt % 4", dict(ldt=10)),
                                      ("maskT not 16-byte aligned", dict(maskT=0x200008))])
def test_the_transpose_is_required_where_it_is_read(lib, what, bad):
    """bpm_attn_bwd_dkv_amask and bpm_attn_maps_amask read maskT (the header's stated choice): they reject a bad one."""
    prob, mp, k = _problem(), _map_problem(), _mask(**bad)
    assert lib.bpm_attn_bwd_dkv_amask(_lib.BPM_F32, C.byref(prob), C.byref(k), 1, 0, None) == ERR_ARG, what
    assert lib.bpm_attn_maps_amask(_lib.BPM_F32, C.byref(mp), C.byref(k), 1, None) == ERR_ARG, what


def test_score_gradient_export_is_refused(lib):
    prob, k = _problem(), _mask()
    prob.S = 12                                              # S % 4 == 0, so the unmasked dQ entry would take dS / Pd
    prob.dS, prob.Pd, prob.xs_b, prob.xs_h, prob.xs_q = 0x300000, 0x400000, 1024, 512, 16
    for fn in (lib.bpm_attn_fwd_amask, lib.bpm_attn_bwd_dq_amask, lib.bpm_attn_bwd_dkv_amask):
        assert fn(_lib.BPM_F32, C.byref(prob), C.byref(k), 1, 0, None) == ERR_ARG


def test_ops_wrappers_check_before_calling():
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.attn_amasks([(torch.zeros(4, 4), 4, torch.zeros(4, 4), 4)])
    with pytest.raises(ValueError, match="one additive mask per problem"):
        ops.attn_fwd_amask(_lib.BPM_F32, [_problem()], ops.attn_amasks([]))


@pytest.mark.parametrize("bias", [True, False])
def test_state_dict_equals_the_reference_layout(bias):
    """bpmult/models/multihead_attention.py:17-38: in_proj_weight [3d, d], in_proj_bias [3d] and out_proj (nn.Linear(d, d,
    bias=bias)); with bias=False in_proj_bias is registered as None and out_proj has no bias."""
    d = 48
    m = MultiheadAttention(d, 4, attn_dropout=0.1, bias=bias)
    want = {"in_proj_weight": (3 * d, d), "out_proj.weight": (d, d)}
    if bias:
        want.update({"in_proj_bias": (3 * d,), "out_proj.bias": (d,)})
    assert {k: tuple(v.shape) for k, v in m.state_dict().items()} == want
    assert {k: tuple(p.shape) for k, p in m.named_parameters()} == want
    assert "in_proj_bias" in m._parameters and (m.in_proj_bias is None) == (not bias)
    assert m.head_dim == 12 and m.scaling == 12 ** -0.5 and m.attn_dropout == 0.1
    if bias:
        assert float(m.in_proj_bias.detach().abs().max()) == 0.0 and float(m.out_proj.bias.detach().abs().max()) == 0.0


def test_refused_constructor_flags_and_shapes():
    with pytest.raises(ValueError, match="add_bias_kv"):
        MultiheadAttention(24, 4, add_bias_kv=True)
    with pytest.raises(ValueError, match="add_zero_attn"):
        MultiheadAttention(24, 4, add_zero_attn=True)
    with pytest.raises(ValueError, match="divisible"):
        MultiheadAttention(25, 4)


def test_no_cpu_path():
    m = MultiheadAttention(24, 4)
    x = torch.zeros(3, 2, 24)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x, x)
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(x, x, x, attn_mask=torch.zeros(3, 3), need_weights=False)
