"""No-GPU check of the grouped-GEMM dispatcher's decision: which kernel family and tile bpm_gemm_grouped picks for the
launch classes csrc/gemm.hip's comments name, and which inputs it rejects.  The answers come from bpm_debug_gemm_choice of
the -DBPM_LAB build (the entry point's own check_group / summarise / choose / check_choice / fill_group, for a device of 256
compute units; nothing is launched).  The expected values were recorded from the dispatcher before it was split into those
steps (profiles/r08_parent_choice_hook.patch gives that tree the same query; tools/gemm_choice.py compares whole grids)."""
import ctypes as C

import pytest

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib
from bpmult_amd._lib import (BPM_BF16, BPM_BF16X3, BPM_F32, F_A_OVERLAP, F_ATOMIC, F_KPAD, GEMM_NN, GEMM_NT, GEMM_TN, OUT_CT, OUT_F32)

NCU = 256
KERNELS = ["dma_0", "dma_1", "dma_2", "dma_3", "dma_4", "dma_tall", "dma_two", "x3_2", "x3_3", "x3_tall", "skinny", "tiled_fast",
           "tiled_bounded", "tn_64", "tn_short", "tn_long"]                      # enum Kernel of csrc/gemm.hip
BF, F32, X3, NT, NN, TN = BPM_BF16, BPM_F32, BPM_BF16X3, GEMM_NT, GEMM_NN, GEMM_TN
XS = {"colsum_a": True}                    # weight gradients that carry the bias column sums

# launch class: (dtype, variant, problems, (M, N, K), fields that differ from a plain F_KPAD product) -> (kernel, bm, bn, workgroups)
ROWS = {
    # hidden 768, six problems of 4096 rows
    "q / out (NT)":                 ((BF, NT, 6, (4096, 768, 768), {}),                    ("dma_tall", 320, 256, 234)),
    "fc2 (NT)":                     ((BF, NT, 6, (4096, 768, 3072), {}),                   ("dma_tall", 320, 256, 234)),
    "fc1 (NT)":                     ((BF, NT, 6, (4096, 3072, 768), {}),                   ("dma_two", 256, 128, 2304)),
    "d(fc2) (NN)":                  ((BF, NN, 6, (4096, 3072, 768), {}),                   ("dma_3", 256, 256, 1152)),
    "d(fc1) (NN)":                  ((BF, NN, 6, (4096, 768, 3072), {}),                   ("dma_tall", 320, 256, 234)),
    "d(out) / d(q) (NN)":           ((BF, NN, 6, (4096, 768, 768), {}),                    ("dma_tall", 320, 256, 234)),
    "K / V projections, twelve":    ((BF, NT, 12, (4096, 768, 768), {}),                   ("dma_two", 256, 128, 1152)),
    # weight gradients
    "fc1 weight gradients (TN)":    ((BF, TN, 6, (3072, 768, 4096), {}),                   ("dma_2", 256, 256, 216)),
    "fc2 weight gradients (TN)":    ((BF, TN, 6, (768, 3072, 4096), {}),                   ("dma_two", 256, 128, 432)),
    "attention weight gradients, 24": ((BF, TN, 24, (768, 768, 4096), XS),                 ("dma_2", 256, 256, 216)),
    "attention weight gradients, 18": ((BF, TN, 18, (768, 768, 4096), XS),                 ("dma_2", 256, 256, 162)),
    "attention weight gradients, 12": ((BF, TN, 12, (768, 768, 4096), XS),                 ("tiled_fast", 128, 64, 864)),
    # hidden 300 (tests/test_kernels_gpu.py::test_gemm_hidden_300_products_take_the_two_resident_tiles)
    "hidden 300, 300 x 300 (NT)":   ((BF, NT, 6, (4000, 300, 300), {"bias_n": True, "resid": True}), ("dma_two", 256, 128, 288)),
    "hidden 300, 300 x 1200 (NT)":  ((BF, NT, 6, (4000, 300, 1200), {"bias_n": True, "resid": True}), ("dma_two", 256, 128, 288)),
    "hidden 300, 300 x 1200 (NN)":  ((BF, NN, 6, (4000, 300, 1200), {"bias_n": True, "resid": True}), ("dma_two", 256, 128, 288)),
    "hidden 300, 300 x 300 (NN)":   ((BF, NN, 6, (4000, 300, 300), {"bias_n": True, "resid": True}), ("dma_two", 256, 128, 288)),
    "hidden 1536 fc1 (K > 1024)":   ((BF, NT, 6, (4096, 6144, 1536), {}),                  ("dma_3", 256, 256, 2304)),
    "16 rows (NT)":                 ((BF, NT, 6, (16, 768, 768), {}),                      ("skinny", 16, 64, 72)),
    "16 rows, f32 (NN)":            ((F32, NN, 6, (16, 768, 768), {}),                     ("skinny", 16, 64, 72)),
    "batched":                      ((BF, NT, 1, (512, 512, 64), {"batch": 96}),           ("tiled_fast", 128, 64, 3072)),
    "split-K weight gradient":      ((BF, TN, 6, (768, 768, 4096), {"splitk": 4, "flags": F_KPAD | F_ATOMIC}), ("tiled_fast", 128, 64, 1728)),
    "split-K, few workgroups":      ((BF, TN, 1, (768, 768, 4096), {"splitk": 4, "flags": F_KPAD | F_ATOMIC}), ("tn_64", 64, 64, 576)),
    "overlapping rows (convolution)": ((BF, NT, 1, (16000, 96, 12288), {"flags": F_KPAD | F_A_OVERLAP, "lda": 192, "bias_n": True}), ("tiled_fast", 128, 64, 250)),
    "f32 (NT)":                     ((F32, NT, 6, (4096, 768, 768), {}),                   ("tiled_fast", 128, 64, 2304)),
    "f32 weight gradients (TN)":    ((F32, TN, 6, (768, 768, 4096), {}),                   ("tn_64", 64, 64, 864)),
    "no F_KPAD (NT)":               ((BF, NT, 6, (4096, 768, 768), {"flags": 0}),          ("tiled_bounded", 128, 64, 2304)),
    "no F_KPAD (TN), 24":           ((BF, TN, 24, (768, 768, 4096), {"flags": 0}),         ("tn_short", 128, 64, 1728)),
    "no F_KPAD (TN), 6":            ((BF, TN, 6, (768, 768, 4096), {"flags": 0}),          ("tn_long", 128, 64, 432)),
    "CT output (NT)":               ((BF, NT, 6, (4096, 768, 768), {"out_kind": OUT_CT}),  ("dma_tall", 320, 256, 234)),
    # split-bf16 operands, leading dimensions as ops._X3Plan lays them out
    "bf16x3 (NT)":                  ((X3, NT, 6, (4096, 768, 768), {}),                    ("x3_tall", 320, 256, 234)),
    "bf16x3 (NN), 3072 columns":    ((X3, NN, 6, (4096, 3072, 768), {}),                   ("x3_3", 256, 256, 1152)),
    "bf16x3 (TN)":                  ((X3, TN, 6, (3072, 768, 4096), {}),                   ("x3_2", 256, 256, 216)),
}

# rejected before anything is launched: -> the entry point's code (-1 = BPM_ERR_ARG, -2 = BPM_ERR_ALIGN)
REJECTED = {
    "no problems":                          ((BF, NT, 0, (4096, 768, 768), {}), -1),
    "rows of 600 bytes":                    ((BF, NT, 6, (4096, 768, 300), {"lda": 300}), -2),
    "A off by 4 bytes":                     ((BF, NT, 6, (4096, 768, 768), {"A_offset": 4}), -2),
    "overlapping rows without F_KPAD":      ((BF, NT, 1, (16000, 96, 12288), {"flags": F_A_OVERLAP, "lda": 192}), -1),
    "split-K without atomics":              ((BF, TN, 6, (768, 768, 4096), {"splitk": 4}), -1),
    "colsum_a outside a weight gradient":   ((BF, NT, 6, (4096, 768, 768), XS), -1),
    "a batch of none":                      ((BF, NT, 1, (512, 512, 64), {"batch": 0}), -1),
    "CT rows wider than the column tiles":  ((BF, NT, 6, (4096, 700, 768), {"out_kind": OUT_CT, "ldc": 1024}), -1),
    "bf16x3 without F_KPAD (only the LDS-DMA kernel computes it)": ((X3, NT, 6, (4096, 768, 768), {"flags": 0}), -1),
    "bf16x3 with a row bias":               ((X3, NT, 6, (4096, 768, 768), {"bias_m": True}), -1),
}


def pad(n, to):
    return (n + to - 1) // to * to


def problems(dtype, variant, count, shape, fields):
    """`count` problems of one shape at made-up (never read) addresses: rows padded to 32 elements, F_KPAD, fp32 output."""
    M, N, K = shape
    f = dict(fields)
    probs = (_lib.GemmProblem * max(count, 1))()
    addr = 0x7F0000000000
    for p in probs:
        ext_a, ext_b = (K if variant != GEMM_TN else M), (K if variant == GEMM_NT else N)
        to = 128 if dtype == BPM_BF16X3 else 32
        planes = 2 if dtype == BPM_BF16X3 else 1                   # [hi plane | lo plane]
        p.M, p.N, p.K = M, N, K
        p.lda, p.ldb, p.ldc = f.get("lda", planes * pad(ext_a, to)), planes * pad(ext_b, to), f.get("ldc", N)
        p.ldr, p.alpha, p.gate_scale = N, 1.0, 1.0
        p.flags, p.out_kind, p.splitk = f.get("flags", F_KPAD), f.get("out_kind", OUT_F32), f.get("splitk", 1)
        for name in ("A", "B", "C") + tuple(k for k in ("bias_n", "bias_m", "resid", "colsum_a") if f.get(k)):
            setattr(p, name, addr + f.get(name + "_offset", 0))
            addr += 1 << 28
        if "batch" in f:
            p.flags |= _lib.F_BATCHED
            p.batch, p.batch_stride_a, p.batch_stride_b, p.batch_stride_c = f["batch"], M * p.lda, N * p.ldb, M * p.ldc
    return probs


@pytest.fixture(scope="module")
def lab():
    _lib.build_lab()
    with _lib.lab_library() as L:
        yield L


def ask(L, dtype, variant, count, shape, fields, ncu=NCU):
    out = (C.c_int * (4 + 4 * max(count, 1)))()
    rc = L.bpm_debug_gemm_choice(dtype, variant, problems(dtype, variant, count, shape, fields), count, ncu, out)
    return rc, out


@pytest.mark.parametrize("name", list(ROWS))
def test_launch_class_takes_its_kernel_and_tile(lab, name):
    (dtype, variant, count, shape, fields), want = ROWS[name]
    rc, out = ask(lab, dtype, variant, count, shape, fields)
    assert rc == 0, rc
    assert (KERNELS[out[0]], out[1], out[2], out[3]) == want
    # the problems' shares of the grid: consecutive, tiles of the chosen size, split-K slices / batches counted
    M, N, _ = shape
    slices = fields.get("batch", fields.get("splitk", 1))
    per = pad(M, out[1]) // out[1] * (pad(N, out[2]) // out[2]) * slices
    assert [tuple(out[4 + 4 * i:8 + 4 * i]) for i in range(count)] == \
           [(i * per, pad(M, out[1]) // out[1], pad(N, out[2]) // out[2], slices) for i in range(count)]


@pytest.mark.parametrize("name", list(REJECTED))
def test_rejected_inputs_and_their_codes(lab, name):
    (dtype, variant, count, shape, fields), want = REJECTED[name]
    rc, _ = ask(lab, dtype, variant, count, shape, fields)
    assert rc == want


def test_the_query_needs_a_device_size_and_the_entry_point_agrees_on_rejections(lab):
    (dtype, variant, count, shape, fields), _ = ROWS["q / out (NT)"]
    assert ask(lab, dtype, variant, count, shape, fields, ncu=0)[0] == -1           # it never asks a device
    for (dtype, variant, count, shape, fields), want in REJECTED.values():         # the same steps run in front of the launch
        assert lab.bpm_gemm_grouped(dtype, variant, problems(dtype, variant, count, shape, fields), count, 0, None) == want
