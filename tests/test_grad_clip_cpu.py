"""No-GPU checks of the gradient-norm / clipping additions: the new struct mirrors the header, the new entries validate
their arguments on the host before anything is launched, and FusedAdam carries `max_grad_norm` in its param group."""
import math
import os
import re
from types import SimpleNamespace

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bpmult_hip.h")).read()


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def _c_fields(struct_name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = decl.split(",")
        names.append(parts[0].split()[-1].lstrip("*"))
        names += [p.strip().lstrip("*") for p in parts[1:]]
    return [re.sub(r"\[\d+\]$", "", n) for n in names]


def test_sumsq_seg_mirrors_the_header():
    assert _c_fields("bpm_sumsq_seg") == [f[0] for f in _lib.SumsqSeg._fields_]
    assert _c_fields("bpm_sumsq_seg") == ["p", "n", "blk0", "pad_"]
    import ctypes as C
    assert C.sizeof(_lib.SumsqSeg) == 24


def test_block_and_workspace_helpers(lib):
    """A segment's windows start at the 16-byte line at or below its first element: 4096 elements per block, counted
    from there.  The workspace holds one float per block, in whole 16-byte quads."""
    assert lib.bpm_grad_sumsq_blocks(0x10000, 1) == 1
    assert lib.bpm_grad_sumsq_blocks(0x10000, 4096) == 1
    assert lib.bpm_grad_sumsq_blocks(0x10000, 4097) == 2
    assert lib.bpm_grad_sumsq_blocks(0x10004, 4096) == 2           # one element past the line: 4097 window slots
    assert lib.bpm_grad_sumsq_blocks(0x1000c, 4093) == 1
    assert lib.bpm_grad_sumsq_blocks(0x1000c, 4094) == 2
    assert lib.bpm_grad_sumsq_ws_bytes(1) == 16 and lib.bpm_grad_sumsq_ws_bytes(4) == 16 and lib.bpm_grad_sumsq_ws_bytes(5) == 32
    from bpmult_amd import ops
    for ptr, n in ((0x10000, 1), (0x10004, 4096), (0x1000c, 4094), (0x10008, 3 * 4096 + 7)):
        dry = ((ptr >> 2 & 3) + n + 4095) // 4096                 # ops' _DRY_RUN branch
        assert lib.bpm_grad_sumsq_blocks(ptr, n) == dry == ops.grad_sumsq_blocks(ptr, n)


def test_new_entries_validate_on_the_host(lib):
    """Made-up aligned addresses: only rejected calls are made here (a call that passes validation launches)."""
    tab, ws, out, extra = 0x10000, 0x20000, 0x30000, 0x40000
    need = lib.bpm_grad_sumsq_ws_bytes(100)
    assert need == 400
    assert lib.bpm_grad_sumsq(None, 1, 100, 1.0, 0.8, None, ws, need, out, None) == -1          # null table
    assert lib.bpm_grad_sumsq(tab, 0, 100, 1.0, 0.8, None, ws, need, out, None) == -1           # no segments
    assert lib.bpm_grad_sumsq(tab, 1, 0, 1.0, 0.8, None, ws, need, out, None) == -1             # zero blocks
    assert lib.bpm_grad_sumsq(tab, 1, 100, 1.0, 0.8, None, None, need, out, None) == -1         # null workspace
    assert lib.bpm_grad_sumsq(tab, 1, 100, 1.0, 0.8, None, ws, need, None, None) == -1          # null output
    assert lib.bpm_grad_sumsq(tab, 1, 100, 1.0, 0.8, None, ws, need - 1, out, None) == -1       # workspace too small
    assert lib.bpm_grad_sumsq(tab, 1, 100, 1.0, 0.8, extra, ws, 0, out, None) == -1
    assert lib.bpm_grad_sumsq(tab, 1, 100, 1.0, 0.8, None, ws + 4, need, out, None) == -2       # misaligned workspace
    assert lib.bpm_grad_sumsq(tab, 1, 100, 1.0, 0.8, None, ws, need, out + 4, None) == -2       # misaligned output
    assert lib.bpm_grad_sumsq(tab, 1, 100, 1.0, 0.8, extra + 2, ws, need, out, None) == -2      # misaligned extra_sumsq
    a = (_lib.BPM_F32, tab, 1, 1, 0x50000, 0x60000, 0x70000, 0x80000, 1e-3, .9, .999, 1e-8, 0.)
    assert lib.bpm_adam_step_table_clip(*a, 0, 1., out + 4, 0, None) == -1                      # step >= 1
    assert lib.bpm_adam_step_table_clip(*a, 0, 1., None, 0, None) == -1
    assert lib.bpm_adam_step_table_clip(_lib.BPM_F32, None, 1, 1, 0x50000, 0x60000, 0x70000, 0x80000, 1e-3, .9, .999, 1e-8, 0.,
                                        1, 1., out + 4, 0, None) == -1                          # null table
    assert lib.bpm_adam_step_table_clip(*a, 1, 1., out + 2, 0, None) == -2                      # misaligned scale
    assert lib.bpm_adam_step_table_clip(_lib.BPM_F32, tab, 1, 1, 0x50000, 0x60004, 0x70000, 0x80000, 1e-3, .9, .999, 1e-8, 0.,
                                        1, 1., out + 4, 0, None) == -2                          # misaligned gradient


def _toy():
    from bpmult_amd.models import get_model
    a = SimpleNamespace(model="mmtrvat", orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=24, vonly=True, lonly=True,
                        aonly=True, num_heads=4, layers=1, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.,
                        res_dropout=0., out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6,
                        bert_model="unused", text_features=True)
    return get_model(a)


@pytest.mark.parametrize("x", [0, -1, float("inf"), float("nan"), 0.0, -0.5, True, "0.8"])
def test_max_grad_norm_is_validated(x):
    from bpmult_amd.optim import FusedAdam
    with pytest.raises(ValueError, match="max_grad_norm"):
        FusedAdam(_toy(), lr=1e-3, max_grad_norm=x)


def test_max_grad_norm_lives_in_the_param_group():
    """... so it is what a checkpoint's param_groups carry, and the optimizer is still one a scheduler accepts."""
    from bpmult_amd.optim import FusedAdam
    model = _toy()
    opt = FusedAdam(model, lr=1e-3, max_grad_norm=0.8)
    assert opt.param_groups[0]["max_grad_norm"] == 0.8 and opt.last_grad_norm is None
    assert FusedAdam(model, lr=1e-3).param_groups[0]["max_grad_norm"] is None
    assert isinstance(opt, torch.optim.Optimizer) and len(opt.param_groups) == 1
    sched = torch.optim.lr_scheduler.ReduceLROnPlateau(opt, "max", patience=0, factor=0.5)
    sched.step(1.0)
    sched.step(0.5)
    assert math.isclose(opt.param_groups[0]["lr"], 5e-4) and opt.param_groups[0]["max_grad_norm"] == 0.8
