"""No-GPU check of what the row-kernel and Adam entry points launch: for every case of tests/rowops_cases.py -- each branch
of each chooser on both sides of its threshold, the grids at and past their caps, the group limit -- the entry's return
code and, per launch, the kernel instantiation, grid, block and last pointer argument.  The answers come from the dry mode
of the -DBPM_LAB build (bpm_debug_rows_dry: the entry runs check, fill and choose, launch() notes instead of launching).
The expected values were recorded from the tree that still had the one csrc/rowops.hip, which
profiles/rowops_parent_dispatch_hook.patch gives the same query (tools/rowops_dispatch.py writes the record)."""
import json
import os

import pytest

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib

import rowops_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "profiles", "rowops_dispatch.json")) as _f:
    RECORD = json.load(_f)


@pytest.fixture(scope="module")
def lab():
    _lib.build_lab()
    with _lib.lab_library() as L:
        yield L


def test_the_record_covers_the_case_table():
    assert list(RECORD) == list(rowops_cases.CASES)


@pytest.mark.parametrize("name", list(rowops_cases.CASES))
def test_entry_launches_what_the_unsplit_file_launched(lab, name):
    assert rowops_cases.run(lab, rowops_cases.CASES[name]) == RECORD[name]


def test_the_normaliser_reads_both_spellings():
    n = rowops_cases.normalise
    assert n("(ln_fwd_vec_kernel<bf16_t, 3>)") == "ln_fwd_vec_kernel<bf16_t,3>"
    assert n("N12_GLOBAL__N_19KernelTagIXadL_ZNS_17ln_fwd_vec_kernelIDF16bLi3EEEvNS_3GrpINS_3LnPEEEifEEEE") == "ln_fwd_vec_kernel<bf16_t,3>"
    assert n("N12_GLOBAL__N_19KernelTagIXadL_ZNS_20kv_source_bwd_kernelILi12ELb1EEEvNS_3GrpINS_3KvPEEEPKfifEEEE") == \
        "kv_source_bwd_kernel<12,true>"
    assert n("N12_GLOBAL__N_19KernelTagIXadL_Z11adam_kernelPfS1_S1_S1_mffffffiEEE") == n("adam_kernel") == "adam_kernel"


def test_dry_mode_is_off_outside_a_query_and_absent_from_the_product(lab):
    assert lab.bpm_debug_rows_last(-1, None, 0, None, None, None) == 0           # run() switched it off and cleared the notes
    _lib.build()
    product = _lib.load(_lib.LIB_PATH)
    assert not hasattr(product, "bpm_debug_rows_dry") and not hasattr(product, "bpm_debug_rows_last")
