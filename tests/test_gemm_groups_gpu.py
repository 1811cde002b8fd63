"""bpm_gemm_grouped on the MI355X with launches of UNEQUAL problems, against fp64 (tests/gemm_cases.py: the cases, the
reference, the guards and the bounds).  What test_kernels_gpu.py leaves open:

* table A: every kernel family the product library picks by itself, each with a launch whose problems differ in shape
  (ragged M, ragged N, a K that is no whole k stage, a single tile; the smallest first and last), so the tile-to-problem
  prefix (tile0 / pick_problem / xcd_remap) is compared against fp64 with totals of every residue mod 8, and with the
  fused epilogues spread over the problems;
* table B: the general (per-element) epilogue with every feature it implements, beside fast-epilogue problems in one grid;
* table C: the time-axis Linear maps as the engine issues them (single-row and single-column problems, row bias through a
  pointer to one element, k rows Td - 1 rows apart).

bf16-operand products with an fp32 output are held to the f32 mode's 2e-5 of the output's scale (the products are exact
in fp32 and the accumulators are fp32); bf16 outputs to one ulp of the element on top of that.  Every output buffer has
guard cells (a row behind row M, columns behind column N) that must come back bit-identical.

Each case asserts the numerics and the guards first, then that the dispatcher sent the launch to the family its row names
at this device's CU count (bpm_debug_gemm_choice of the lab build on the launch's real problem array); the launch itself
always runs in the product library.  The worst err / bound of every case goes to gemm_group_errors.json beside the
whole-model parity log of test_model_gpu.py (committed copy: profiles/gemm_group_errors.json)."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as G  # noqa: E402
from bpmult_amd import _lib  # noqa: E402

from test_model_gpu import PARITY_LOG  # noqa: E402

ERROR_LOG = os.path.join(os.path.dirname(PARITY_LOG), "gemm_group_errors.json")      # the directory the measured-error logs go to
_ERRORS = {}


def _record(case, rec):
    _ERRORS[case.id] = rec
    try:
        os.makedirs(os.path.dirname(ERROR_LOG), exist_ok=True)
        old = {}
        if os.path.exists(ERROR_LOG):
            with open(ERROR_LOG) as f:
                old = json.load(f)
        old.update(_ERRORS)
        with open(ERROR_LOG, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


@pytest.mark.parametrize("case", G.TABLES, ids=[c.id for c in G.TABLES])
def test_group_against_fp64(case):
    hs = G.make_host(case)
    try:
        got, arr = G.launch(case, hs)
    except RuntimeError as e:
        if "HIP error" in str(e) or "illegal memory access" in str(e):       # a faulted device runs nothing more in this session
            pytest.exit(f"{case.id}: GPU fault: {e}", returncode=3)
        raise
    worst, fails, parts = G.check(case, hs, got)
    print(f"{case.id}: worst err / bound = {worst:.4g} {parts}")
    rec = {"worst_err_over_bound": worst, "by_kind": parts, "problems": len(case.probs)}
    _record(case, rec)
    assert not fails, "\n".join(fails)
    assert worst <= 1.0
    if not os.path.exists(_lib.LAB_LIB_PATH):
        pytest.skip("family not verified")
    name, tiles, total = G.family(case, torch.cuda.get_device_properties(0).multi_processor_count, arr)
    _record(case, dict(rec, family=name, tiles=total))
    assert name == case.family_name, f"{case.id}: the dispatcher picked {name}, the row names {case.family_name}"
