"""The grouped-GEMM launch tables of tests/gemm_cases.py without a GPU.

1. Family table: every row of tables A-C, at made-up addresses, is put to bpm_debug_gemm_choice of the -DBPM_LAB build for a
   device of 256 compute units and must land on the kernel family its row names; the rows together must contain every
   (family, variant) pair the product library can pick by itself, keep the shape rules of a row (unequal problems, ragged
   M / N / K, a single tile, the smallest first and last) and give total tile counts of every residue mod 8.  A later
   change of a dispatcher threshold then cannot silently take a family out of tests/test_gemm_groups_gpu.py.
2. Checker self-test: the fp32 CPU emulation of the documented arithmetic (fp32 matmul of the rounded operands, fp32
   epilogue, bf16 rounding at the store) must pass the checker on every row, and must FAIL it with each of eight defects
   injected one at a time -- the evidence that the reference alone stays inside the bounds and that the bounds notice what
   they are meant to.
3. Engine signatures: every bpm_gemm_grouped launch table of a forward + backward of the 3-modal and the 4-modal model at
   hidden 768, batch 8, bf16, pruned and dense (built from host tensors, ops._DRY_RUN), reduced to (variant, family at 256
   CUs, epilogue features of its problems, shapes differ), must occur in tables A-C."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import gemm_cases as G
from bpmult_amd import _lib, ops
from bpmult_amd._lib import (BPM_BF16, F_A_OVERLAP, F_ACCUM, F_ATOMIC, F_B_OVERLAP, F_BATCHED, F_CT_NARROW, F_RELU, GEMM_NN, GEMM_NT, GEMM_TN,
                             OUT_CT, OUT_F32, GemmProblem)

NCU = 256


@pytest.fixture(scope="module", autouse=True)
def lab_build():
    _lib.build_lab()


# ---------------------------------------------------------------------------
# 1. family table
# ---------------------------------------------------------------------------
@pytest.mark.parametrize("case", G.TABLES, ids=[c.id for c in G.TABLES])
def test_row_takes_the_family_it_names_at_256_cus(case):
    name, tiles, total = G.family(case, NCU)
    assert name == case.family_name
    assert [t[0] for t in tiles] == [sum(a * b * c for _, a, b, c in tiles[:i]) for i in range(len(tiles))]     # consecutive shares of the grid
    assert total == sum(a * b * c for _, a, b, c in tiles)


def test_table_a_holds_every_family_the_product_library_picks():
    assert {(c.family_name, c.variant) for c in G.TABLE_A} >= G.TABLE_A_PAIRS
    assert {c.family_name for c in G.TABLE_B} == {"tiled_fast", "tiled_bounded", "skinny"}
    assert {c.dtype for c in G.TABLE_B} == {_lib.BPM_F32, BPM_BF16}


# `big` (csrc/gemm.hip::summarise) needs N >= 256, two of the 128-column tiles of the two-resident configuration
NO_SINGLE_TILE = {"A/dma_two/NT/twelve", "A/dma_two/NT/wide", "A/dma_two/TN"}


@pytest.mark.parametrize("case", G.TABLE_A + G.TABLE_B, ids=[c.id for c in G.TABLE_A + G.TABLE_B])
def test_row_keeps_the_shape_rules(case):
    name, tiles, _ = G.family(case, NCU)
    bm, bn = {"dma_3": (256, 256), "dma_2": (256, 256), "dma_tall": (320, 256), "dma_two": (256, 128), "x3_3": (256, 256), "x3_2": (256, 256),
              "x3_tall": (320, 256), "skinny": (16, 64), "tn_64": (64, 64)}.get(name, (128, 64))
    qs = case.probs
    assert len(qs) >= 4 and len({(q.M, q.N, q.K) for q in qs}) == len(qs)
    assert any(q.M % bm for q in qs), "a problem ragged in M"
    assert any(q.N % bn and q.N % 4 == 0 for q in qs), "a problem ragged in N with N % 4 == 0"
    assert any(q.K % 32 for q in qs), "a K that is no whole k stage"
    count = [a * b * c for _, a, b, c in tiles]
    assert [(q.M + bm - 1) // bm * ((q.N + bn - 1) // bn) * q.splitk for q in qs] == count
    assert case.name in NO_SINGLE_TILE or 1 in count, "a single-tile problem"
    assert count[0] == count[-1] == min(count), "the first and the last problem are the smallest"


def test_total_tile_counts_take_every_residue_mod_8():
    totals = [G.family(c, NCU)[2] for c in G.TABLES]
    assert {t % 8 for t in totals} == set(range(8)) and min(totals) < 8          # xcd_remap: q = total >> 3, r = total & 7
    a = {c.name: n for c, n in zip(G.TABLES, totals)}
    assert len({a[c.name] % 8 for c in G.TABLE_A}) >= 6


def test_skinny_rows_cover_one_to_sixteen_rows():
    for c in G.TABLE_A:
        if c.family_name == "skinny":
            ms = {q.M for q in c.probs}
            assert {1, 16} <= ms and max(ms) == 16 and len(ms) >= 7


# ---------------------------------------------------------------------------
# 2. checker self-test
# ---------------------------------------------------------------------------
# (the emulation restates the f32 / bf16 kernels; of the LDS-DMA rows, whose host data take seconds, one stands for all:
#  the checker does not know the family)
EMULATED = [c for c in G.TABLES if not c.x3 and (not c.family_name.startswith("dma") or c.name == "A/dma_3/NT")]
_HOST = {}


def host(case):                                       # one set of inputs + reference per row, shared by the tests below
    if case.id not in _HOST:
        _HOST[case.id] = G.make_host(case)
    return _HOST[case.id]


@pytest.mark.parametrize("case", EMULATED, ids=[c.id for c in EMULATED])
def test_checker_accepts_the_fp32_emulation(case):
    hs = host(case)
    worst, fails, parts = G.check(case, hs, G.emulate(case, hs))
    assert not fails and worst <= 1.0, fails
    # an fp32 output of the emulation sits far inside the bound: the reference arithmetic is not what fills it
    assert parts.get("fp32_out", 0.0) < 0.5 and parts.get("colsum", 0.0) < 0.5


def test_one_mixed_shape_case_per_output_kind():
    for c in SELF_TEST:
        assert c.shapes_differ() and {q.out for q in c.probs} >= {"f32", "ct", "narrow", "heads"}


SELF_TEST = [c for c in G.TABLES if c.id in ("A/tiled_fast/NT-bf16", "B/tiled_fast/NT-bf16", "A/dma_3/NT-bf16")]


@pytest.mark.parametrize("defect", list(G.DEFECTS))
@pytest.mark.parametrize("case", SELF_TEST, ids=[c.id for c in SELF_TEST])
def test_checker_rejects_an_injected_defect(case, defect):
    hs = host(case)
    worst, fails, _ = G.check(case, hs, G.emulate(case, hs, defect))
    assert fails, f"{defect}: passed with worst err / bound = {worst:.3g}"
    assert len(fails) <= 2, fails                     # one defect, one problem: nothing else may trip


# ---------------------------------------------------------------------------
# 3. the signatures the engine launches
# ---------------------------------------------------------------------------
def _model_args(model, prune):
    four = model == "mmtrvapt"
    return SimpleNamespace(model=model, hidden_sz=768, num_heads=6 if four else 12, layers=3, n_classes=13 if four else 6, orig_d_l=768,
                           orig_d_v=4096 if four else 35, orig_d_a=96 if four else 74, orig_d_p=4096, vonly=True, lonly=True, aonly=True,
                           attn_dropout=0.1, attn_dropout_v=0.0, attn_dropout_a=0.0, relu_dropout=0.1, res_dropout=0.1, out_dropout=0.0,
                           embed_dropout=0.25, attn_mask=True, hybrid=False, bert_model="unused", text_features=True, precision="bf16",
                           num_vectors_l=512, num_vectors_a=200 if four else 512, num_vectors_v=200 if four else 512,
                           prune_unused_rows=prune)


def _walk(obj, out, seen):
    """Every (ops.gemm_grouped, dtype, variant, problems) step inside nested step tables."""
    if id(obj) in seen or isinstance(obj, (torch.Tensor, str, bytes, int, float)):
        return
    seen.add(id(obj))
    if isinstance(obj, tuple) and obj and obj[0] is ops.gemm_grouped:
        out.append((obj[2], obj[3]))
    elif isinstance(obj, (list, tuple)):
        for x in obj:
            _walk(x, out, seen)
    elif isinstance(obj, dict):
        for x in obj.values():
            _walk(x, out, seen)


def engine_launches(model, prune, B=8):
    """[(variant, problem array)] of every grouped-GEMM launch table of the trunk: the encoder plans' forward / backward step
    tables, the Fusion-GMU and time-map tables and the 1x1 input projections (recorded from conv_forward / conv_backward).
    Needs ops._DRY_RUN (host tensors stand in for device buffers; nothing is launched)."""
    from bpmult_amd.models import get_model
    m = get_model(_model_args(model, prune))
    m._ensure_store()
    trunk = m._trunk_for(B)
    out = []
    for plan in (trunk.plan1, trunk.plan2):
        _walk(vars(plan), out, set())
    out += [(GEMM_NT, trunk._gmu_fwd[1]), (GEMM_TN, trunk._gmu_bwd[1]), (GEMM_NN, trunk._gmu_bwd[2]), (GEMM_NN, trunk._gmu_bwd[3])]
    if trunk.tmap:
        out += [(GEMM_NN, trunk._time_fwd[1]), (GEMM_NT, trunk._time_bwd[1]), (GEMM_TN, trunk._time_bwd[2])]
    # the input projections build their problems per call: record them
    saved = {n: getattr(ops, n) for n in ("gemm_grouped", "pack_rows_fwd", "pack_rows_bwd", "rows_cast")}
    try:
        for n in saved:
            setattr(ops, n, lambda *a, **k: None)
        ops.gemm_grouped = lambda dtype, variant, probs, seed=0, n=None, x3=False: out.append((variant, ops.array(GemmProblem, probs)))
        a = _model_args(model, prune)
        feats = {"l": torch.zeros(B, 20, a.orig_d_l), "v": torch.zeros(B, 100, a.orig_d_v), "a": torch.zeros(B, 90, a.orig_d_a)}
        trunk.conv_forward(feats, 0, True)
        trunk.conv_backward(0, {"l": True, "v": True, "a": True})
    finally:
        for n, f in saved.items():
            setattr(ops, n, f)
    return [(v, arr) for v, arr in out if len(arr)]


def _features(p):
    f = {n for n in ("bias_n", "bias_m", "resid", "gate", "colsum", "colsum_a") if getattr(p, n)}
    f |= {n for n, bit in (("accum", F_ACCUM), ("atomic", F_ATOMIC), ("relu", F_RELU), ("narrow", F_CT_NARROW), ("batched", F_BATCHED),
                           ("overlap", F_A_OVERLAP | F_B_OVERLAP)) if p.flags & bit}
    f |= ({"alpha"} if p.alpha != 1.0 else set()) | ({"drop"} if p.drop_p > 0 else set()) | ({"splitk"} if p.splitk > 1 else set())
    return frozenset(f | {"out_f32" if p.out_kind == OUT_F32 else "out_ct" if p.out_kind == OUT_CT else "out_heads"})


def signature(variant, arr, dtype=BPM_BF16):
    """(variant, family at 256 CUs, the set of epilogue feature sets over the launch's problems, shapes differ)."""
    n = len(arr)
    res = (C.c_int * (4 + 4 * n))()
    with _lib.lab_library() as L:
        rc = L.bpm_debug_gemm_choice(dtype, variant, arr, n, NCU, res)
    assert rc == 0, rc
    return (G.VNAME[variant], G.KERNELS[res[0]], frozenset(_features(p) for p in arr), len({(p.M, p.N, p.K) for p in arr}) > 1)


def _table_signatures():
    rows = []
    for c in G.TABLES:
        if c.dtype == BPM_BF16:
            rows.append((G.VNAME[c.variant], c.family_name, [frozenset(c.features(q)) for q in c.probs], c.shapes_differ()))
    return rows


def covered(sig, rows=None):
    """A launch signature occurs in the tables when a row of its variant and family, with unequal problems if the launch has
    them, holds for every feature set of the launch a problem with exactly those features or with those and more (the row
    spreads all its family's epilogues over its problems; a problem that adds alpha to `bias_n -> heads` runs the same code)."""
    variant, fam, feats, differ = sig
    for v, f, row_feats, row_differ in rows or _table_signatures():
        if (v, f) == (variant, fam) and (row_differ or not differ) and all(any(x <= y for y in row_feats) for x in feats):
            return True
    return False


# Signatures that no small launch reproduces, by name, with the reason
NOT_REPRODUCED = {
    # the low-rank key side of the pruned 3-modal model: BPM_GEMM_BATCHED problems (with CT_NARROW outputs) beside plain
    # ones.  Batched problems are outside these tables; tests/test_kernels_gpu.py::test_gemm_batched_problems_with_interleaved_rows
    # runs exactly this pairing (a batched NN / TN problem beside a plain one) against fp64
    "batched problems (low-rank key side)": lambda sig: any("batched" in f for f in sig[2]),
}


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    try:
        yield
    finally:
        ops._DRY_RUN = False


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "dense"])
@pytest.mark.parametrize("model", ["mmtrvat", "mmtrvapt"])
def test_every_engine_launch_signature_occurs_in_the_tables(dry_run, model, prune):
    launches = engine_launches(model, prune)
    assert len(launches) > 40
    rows = _table_signatures()
    missing = set()
    for variant, arr in launches:
        sig = signature(variant, arr)
        if not covered(sig, rows) and not any(why(sig) for why in NOT_REPRODUCED.values()):
            missing.add((sig[0], sig[1], tuple(sorted(tuple(sorted(x)) for x in sig[2])), sig[3]))
    assert not missing, "\n".join(map(str, sorted(missing)))
