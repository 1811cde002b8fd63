"""No-GPU check of what the attention entry points launch: for every case of tests/attn_cases.py -- each entry at each
compute type and padded head_dim, both block-pairing settings, the dS / Pd export, groups up to and past the limit, the
maps and bias-gradient choosers on both sides of their thresholds, one case per refusal and a few with two faults -- the
entry's return code and, per launch, the kernel instantiation, grid and block.  The answers come from the dry mode of the
-DBPM_LAB build (bpm_debug_rows_dry: the entry runs check, fill and choose, launch() notes instead of launching).
The expected values were recorded from the tree that still had all of attention in the one csrc/attention.hip, whose
launches profiles/attn_parent_dispatch_hook.patch routes to the same query (`tools/rowops_dispatch.py --cases attn` writes
the record)."""
import json
import os

import pytest

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib

import attn_cases

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
with open(os.path.join(ROOT, "profiles", "attn_dispatch.json")) as _f:
    RECORD = json.load(_f)


@pytest.fixture(scope="module")
def lab():
    _lib.build_lab()
    with _lib.lab_library() as L:
        yield L


def test_the_record_covers_the_case_table():
    assert list(RECORD) == list(attn_cases.CASES)


@pytest.mark.parametrize("name", list(attn_cases.CASES))
def test_entry_launches_what_the_unsplit_file_launched(lab, name):
    assert attn_cases.run(lab, attn_cases.CASES[name]) == RECORD[name]


def test_dry_mode_is_off_outside_a_query_and_absent_from_the_product(lab):
    assert lab.bpm_debug_rows_last(-1, None, 0, None, None, None) == 0           # run() switched it off and cleared the notes
    _lib.build()
    product = _lib.load(_lib.LIB_PATH)
    assert not hasattr(product, "bpm_debug_rows_dry") and not hasattr(product, "bpm_debug_rows_last")
    assert not hasattr(product, "bpm_debug_attn_pair")
