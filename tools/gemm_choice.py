"""Which kernel and tile bpm_gemm_grouped chooses, on the CPU: no GPU, nothing launched.

Every case is one grouped-GEMM call; its answer comes from bpm_debug_gemm_choice of the -DBPM_LAB build (the dispatcher's
own check / summarise / choose / fill steps for a device of --ncu compute units): the code the entry point would return
up to the launch, the kernel family (enum Kernel of csrc/gemm.hip), the tile, the grid and each problem's share of it.

  (a) the model's launches: every bpm_gemm_grouped call of one eager training step from host tensors (the stand-in
      library of tools/step_trace.py), bench.py's configurations, bf16 and f32, pruned and dense schedule, with the
      4-modal model's AudioEncoder and poster products.  The bf16x3 mode needs a device; (b) covers its launches.
  (b) a seeded synthetic grid: shapes, group sizes, flags, split-K, optional pointers present / absent / misaligned,
      leading dimensions exact / padded / short, split-bf16 operands as ops._X3Plan lays them out, invalid groups.
  (c) the same under every bpm_debug_gemm_force setting.

    python tools/gemm_choice.py > a.txt              one JSON line per case, then the summary line
    python tools/gemm_choice.py --summary            the summary line only: case count, cases per kernel and per code, SHA-256
    python tools/gemm_choice.py --lib other_lab.so   another build of the library (a parent with the same query patched in)

Pointers are printed as null or their value mod 16, so two trees that decide alike print the same bytes."""
import argparse
import ctypes as C
import gc
import hashlib
import json
import os
import random
import sys

import torch

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
sys.path.insert(0, ROOT)
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))
import bench  # noqa: E402
import step_trace  # noqa: E402
import bpmult_amd  # noqa: E402,F401
from bpmult_amd import _lib, engine, frontend, ops  # noqa: E402
from bpmult_amd._lib import (BPM_BF16, BPM_BF16X3, BPM_F32, F_A_OVERLAP, F_ACCUM, F_ATOMIC, F_B_OVERLAP, F_BACKGROUND, F_BATCHED,  # noqa: E402
                             F_CT_NARROW, F_KPAD, F_RELU, GEMM_NN, GEMM_NT, GEMM_TN, OUT_CT, OUT_F32, OUT_HEADS, GemmProblem)

KERNELS = ["dma_0", "dma_1", "dma_2", "dma_3", "dma_4", "dma_tall", "dma_two", "x3_2", "x3_3", "x3_tall", "skinny", "tiled_fast",
           "tiled_bounded", "tn_64", "tn_short", "tn_long"]                      # enum Kernel of csrc/gemm.hip


class Probe:
    """Asks the library under test about every case and prints / digests the answers."""

    def __init__(self, path, ncu, quiet):
        self.lab = C.CDLL(path)
        self.lab.bpm_debug_gemm_choice.argtypes = [C.c_int, C.c_int, C.POINTER(GemmProblem), C.c_int, C.c_int, C.POINTER(C.c_int)]
        self.lab.bpm_debug_gemm_force.argtypes = [C.c_int]
        self.ncu, self.quiet = ncu, quiet
        self.sha = hashlib.sha256()
        self.cases, self.kernels, self.codes = 0, {}, {}

    def ask(self, label, dtype, variant, probs, n):
        out = (C.c_int * (4 + 4 * max(n, 0)))()
        rc = self.lab.bpm_debug_gemm_choice(dtype, variant, probs, n, self.ncu, out)
        rec = {"case": label, "dtype": dtype, "variant": variant, "nprob": n, "rc": rc,
               "probs": [self._problem(probs[i]) for i in range(n if probs is not None and 0 <= n <= _lib.GEMM_MAX_GROUP else 0)]}
        if rc == 0:
            rec.update(kernel=KERNELS[out[0]], bm=out[1], bn=out[2], total_tiles=out[3],
                       tiles=[[out[4 + 4 * i + j] for j in range(4)] for i in range(n)])            # tile0, tiles_m, tiles_n, splitk
            self.kernels[rec["kernel"]] = self.kernels.get(rec["kernel"], 0) + 1
        self.codes[str(rc)] = self.codes.get(str(rc), 0) + 1
        self.cases += 1
        line = json.dumps(rec, sort_keys=True, separators=(",", ":"))
        self.sha.update(line.encode() + b"\n")
        if not self.quiet:
            print(line)

    @staticmethod
    def _problem(p):
        out = {}
        for field, ty in GemmProblem._fields_:
            v = getattr(p, field)
            out[field] = (None if not v else v % 16) if ty is C.c_void_p else v
        return out

    def summary(self):
        return {"ncu": self.ncu, "cases": self.cases, "kernels": dict(sorted(self.kernels.items())), "codes": dict(sorted(self.codes.items())),
                "sha256": self.sha.hexdigest()}


# ---- (a) the model's launches -------------------------------------------------------------------------------------------
class StandIn:
    """Stands in for the loaded library (tools/step_trace.py): launches nothing; GEMM calls go to the probe."""

    def __init__(self, probe):
        self.probe, self.label, self.count = probe, "", 0

    def __getattr__(self, name):
        if not name.startswith("bpm_"):
            raise AttributeError(name)
        if name in step_trace.SIZES:
            return step_trace.SIZES[name]
        if name == "bpm_gemm_grouped":
            return self._gemm
        return lambda *a: 0

    def _gemm(self, dtype, variant, probs, n, seed, stream):
        self.probe.ask(f"{self.label} #{self.count}", dtype, variant, probs, n)
        self.count += 1
        return 0


class _OnDevice(torch.Tensor):
    """A host tensor the two front-end entry points take for a device tensor (they refuse host tensors by is_cuda)."""
    is_cuda = True


# (two layers of cfg4 and cfg5: a dense f32 step of either at full depth does not fit 64 GB of host memory; the layers repeat)
MODEL_CASES = [("h768", {}), ("cfg1", {}), ("cfg3", {}), ("k768", {}), ("cfg4", {"layers": 2}), ("cfg5", {"layers": 2})]


def model_launches(probe):
    stand = StandIn(probe)
    _lib._lib = stand
    ops._DRY_RUN = True
    ops._stream = frontend._s = lambda: 0
    ws = torch.zeros(1 << 14)
    ops._ln_workspace = lambda n, d, device: ws
    torch.cuda.current_device = lambda: 0
    engine._SIDE = False
    crit = torch.nn.BCEWithLogitsLoss()
    for name, over in MODEL_CASES:
        c = dict(bench.CONFIGS[name], **over)
        for prec in ("bf16", "f32"):
            for prune in (True, False):
                torch.manual_seed(1234)
                m = bench.make_model(c, prec).train()
                m.use_graphs = False
                m.set_prune_unused_rows(prune)
                b = bench.synth_batch(c, c["batch"], 1234, "cpu")
                for k in ("aud", "post"):
                    if k in b and "post" in b:
                        b[k] = b[k].as_subclass(_OnDevice)
                stand.label, stand.count = f"{name} {prec} prune={prune}", 0
                crit(bench.run_model(m, b), b["tgt"]).backward()
                del m, b
                gc.collect()


# ---- (b) the synthetic grid ---------------------------------------------------------------------------------------------
DIMS = [1, 16, 17, 64, 200, 255, 256, 300, 384, 768, 1000, 1024, 1536, 2048, 3072, 4096, 6144]
FLAGS = [0, F_ACCUM, F_RELU, F_ATOMIC, F_KPAD, F_BACKGROUND, F_A_OVERLAP, F_B_OVERLAP, F_CT_NARROW, F_BATCHED,           # singly
         F_KPAD | F_RELU, F_KPAD | F_ACCUM, F_KPAD | F_BACKGROUND, F_KPAD | F_ACCUM | F_BACKGROUND, F_KPAD | F_A_OVERLAP,
         F_KPAD | F_B_OVERLAP, F_KPAD | F_A_OVERLAP | F_B_OVERLAP, F_KPAD | F_CT_NARROW, F_KPAD | F_BATCHED, F_KPAD | F_ATOMIC,
         F_ACCUM | F_ATOMIC]                                                                                              # as the engine combines them
BASE = 0x7F0000000000                      # addresses are compared, aligned and never read


def pad(n, to):
    return (n + to - 1) // to * to


def grid_group(rng, dtype, variant, nprob):
    """One group the way the engine builds them: its problems share flags and layout, and half of the groups their shape.
    ALIGNMENT: what the entry point answers with the alignment code (an A / B address off by 4 bytes, a leading dimension
    that is no multiple of 16 bytes) sits in problem 0 or in every problem of a one-shape group, and never in a split-bf16
    group.  A group with an alignment fault BEHIND a problem whose fault depends on the chosen tile (a CT output wider than
    its column tiles, a batched problem on a tile that takes none, split operands the LDS-DMA kernel refuses) reports
    whichever of the two the dispatcher meets first; the check order is its own business, so the grid keeps such double
    faults out."""
    x3 = dtype == BPM_BF16X3
    flags = rng.choice(FLAGS) if rng.random() < 0.5 else F_KPAD
    ld_mode = rng.choice(["exact", "pad32", "pad32", "pad128", "short"])
    out_kind = rng.choice([OUT_F32, OUT_F32, OUT_CT, OUT_HEADS])
    splitk = 4 if rng.random() < 0.15 else 1
    if splitk > 1 and rng.random() < 0.7:
        flags, out_kind = flags | F_ATOMIC, OUT_F32
    present = {k: rng.random() < p for k, p in (("bias_n", .4), ("bias_m", .05), ("resid", .2), ("gate", .2), ("colsum", .2), ("colsum_a", .25))}
    offset = {k: 4 if rng.random() < 0.08 else 0 for k in ("C", "bias_n", "bias_m", "resid", "gate", "colsum", "colsum_a")}
    shape = [rng.choice(DIMS) for _ in range(3)]
    defect = rng.choice(["null_a", "zero_m", "heads", "batch", "ld_odd", "a_off", "b_off"]) if rng.random() < 0.1 else None
    if x3 and defect in ("ld_odd", "a_off", "b_off"):       # (see ALIGNMENT below)
        defect = None
    mixed = ld_mode != "exact" and rng.random() < 0.5
    probs = (GemmProblem * max(nprob, 1))()
    addr = BASE
    for i in range(nprob):
        p = probs[i]
        M, N, K = [rng.choice(DIMS) for _ in range(3)] if mixed and rng.random() < 0.4 else shape
        p.M, p.N, p.K = M, N, K
        ext_a, ext_b = (K if variant != GEMM_TN else M), (K if variant == GEMM_NT else N)      # the contiguous extent of A and B rows
        if x3:                                                                                  # ops._X3Plan: [hi plane | lo plane]
            p.lda, p.ldb = 2 * pad(ext_a, 128), 2 * pad(ext_b, 128)
            if ld_mode == "short":
                p.lda -= 128
        else:
            to = {"exact": 1, "pad32": 32, "pad128": 128, "short": 32}[ld_mode]
            p.lda, p.ldb = pad(ext_a, to), pad(ext_b, to)
            if ld_mode == "short":
                p.lda, p.ldb = max(p.lda - 32, 8), max(p.ldb - 32, 8)
        if flags & F_A_OVERLAP:
            p.lda = 192                                                                        # a convolution's row stride
        if flags & F_B_OVERLAP:
            p.ldb = 192
        p.ldc = rng.choice([N, pad(N, 32), pad(N, 32), pad(N, 128), pad(N, 256)])
        p.ldr, p.ldg = pad(N, 4) if rng.random() < 0.9 else N, pad(N, 32)
        for k in ("A", "B", "C"):
            setattr(p, k, addr + offset.get(k, 0))
            addr += 1 << 24
        for k, on in present.items():
            if on:
                setattr(p, k, addr + offset[k])
                addr += 1 << 24
        p.gate_scale, p.alpha = 1.0, 1.0
        p.drop_p, p.drop_site = (0.1, i) if rng.random() < 0.2 else (0.0, 0)
        p.flags, p.out_kind, p.splitk = flags, out_kind, splitk if rng.random() < 0.9 else 1
        if out_kind == OUT_HEADS:
            dh = next((d for d in (64, 32, 16, 8, 4, 1) if N % d == 0))
            p.heads_B, p.heads_H, p.heads_T, p.heads_dh, p.heads_dhp = 8, N // dh, max(M // 8, 1), dh, pad(dh, 32)
        if flags & F_BATCHED:
            p.batch, p.batch_stride_a, p.batch_stride_b, p.batch_stride_c = rng.choice([1, 8, 96, 4096]), 8 * p.lda, 8 * p.ldb, 4 * p.ldc
        if i == 0 and defect == "ld_odd":
            p.lda += 2
        elif i == 0 and defect in ("a_off", "b_off"):
            p.A, p.B = p.A + 4 * (defect == "a_off"), p.B + 4 * (defect == "b_off")
        elif i == (nprob - 1) // 2:                                                            # the other defects sit in one problem
            if defect == "null_a":
                p.A = 0
            elif defect == "zero_m":
                p.M = 0
            elif defect == "heads":
                p.out_kind, p.heads_B, p.heads_H, p.heads_dh = OUT_HEADS, 8, 5, 7
            elif defect == "batch":
                p.flags |= F_BATCHED
                p.batch = rng.choice([0, 5000])
    return probs


def grid(probe, cases, seed):
    rng = random.Random(seed)
    for n in range(cases):
        dtype = rng.choice([BPM_F32, BPM_BF16, BPM_BF16, BPM_BF16X3])
        variant = rng.choice([GEMM_NT, GEMM_NN, GEMM_TN])
        nprob = rng.choice([1, 6, 12, 18, 24])
        probs = grid_group(rng, dtype, variant, nprob)
        bad = rng.random()
        if bad < 0.01:
            nprob = rng.choice([0, -1, _lib.GEMM_MAX_GROUP + 1])
        elif bad < 0.02:
            variant = 3
        elif bad < 0.03:
            dtype = 5
        probe.ask(f"grid {n}", dtype, variant, None if bad > 0.995 else probs, nprob)


def forced(probe, cases, seed):
    """(c): the lab override in front of the automatic choice, every setting."""
    rng = random.Random(seed)
    for cfg in (-2, 0, 1, 2, 3, 4, 5, 6):
        assert probe.lab.bpm_debug_gemm_force(cfg) == 0
        for n in range(cases):
            dtype = rng.choice([BPM_F32, BPM_BF16, BPM_BF16, BPM_BF16X3])
            variant = rng.choice([GEMM_NT, GEMM_NN, GEMM_TN])
            nprob = rng.choice([1, 6, 12])
            probe.ask(f"force {cfg} {n}", dtype, variant, grid_group(rng, dtype, variant, nprob), nprob)
    assert probe.lab.bpm_debug_gemm_force(-1) == 0


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--lib", default=_lib.LAB_LIB_PATH, help="the -DBPM_LAB build to ask")
    ap.add_argument("--ncu", type=int, default=256, help="compute units of the device to decide for")
    ap.add_argument("--summary", action="store_true", help="the summary line only")
    ap.add_argument("--grid", type=int, default=20000, help="synthetic cases")
    ap.add_argument("--no-model", action="store_true", help="skip (a): the full-size model steps take minutes")
    opt = ap.parse_args()
    probe = Probe(opt.lib, opt.ncu, opt.summary)
    grid(probe, opt.grid, 20260)
    forced(probe, opt.grid // 40, 20261)
    if not opt.no_model:
        model_launches(probe)
    missing = [k for k in KERNELS if k not in probe.kernels] + [c for c in ("0", "-1", "-2") if c not in probe.codes]
    print(json.dumps(dict(probe.summary(), missing=missing), sort_keys=True))


if __name__ == "__main__":
    main()
