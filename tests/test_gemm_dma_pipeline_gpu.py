"""The stage ring of the LDS-DMA GEMM (csrc/gemm_dma.h) at the K extents where it can go wrong, for the k-strided forms.

The k loop keeps NS stages in flight with nothing but hand-placed synchronisation (a counted `s_waitcnt vmcnt(N)`, one raw
barrier per stage): the LDS-DMA pieces are issued from inline asm that the compiler's wait-count pass does not see, so a
wrong count or a misplaced barrier is no longer covered by a compiler-inserted drain.  What such a mistake does is read a
stage one iteration early (the bytes of the stage that lived in that buffer before) or late.  So

* configurations: every LDS-DMA configuration with a k-strided form -- dma_2 (256 x 256, 8 waves, 2 stages of 64 k), dma_3
  (256 x 256, 16 waves), dma_tall (320 x 256, NN only), dma_two (256 x 128, 3 stages of 32 k, two workgroups per CU) --
  pinned through bpm_debug_gemm_force of the -DBPM_LAB build, for TN and NN in bf16, plus one bf16x3 launch (x3_3, NN:
  three passes over the ring) by the automatic choice;
* K: one to five stages of the configuration, 72 and 200 (no whole stage), which includes one stage beyond the ring depth
  (3 stages at NS = 2, 4 at NS = 3); every launch holds two problems of DIFFERENT K, one or two tiles each (M, N <= 512);
* operands: random data plus a constant block per stage, another constant for every stage, on both operands: a stage
  read early or late, or twice, moves every output element by far more than the bound;
* reference and bounds: fp64 on the rounded operands, the bounds of tests/test_gemm_groups_gpu.py (gemm_cases.check:
  fp32 outputs 2e-5 of the output's scale, bf16x3 5e-5, column sums 2e-5 of the column's mass), guard cells included;
* every launch runs twice on fresh buffers and the two results are compared bitwise;
* one launch per weight-gradient configuration carries the bias column sums (colsum_a: the XS instantiations)."""
import ctypes as C

import pytest
import torch

pytestmark = pytest.mark.gpu

import gemm_cases as G  # noqa: E402
from bpmult_amd import _lib  # noqa: E402
from bpmult_amd._lib import BPM_BF16, BPM_F32  # noqa: E402
from gemm_cases import NN, TN, P, Case  # noqa: E402

# configuration -> (index for bpm_debug_gemm_force, k per stage, ring depth)
CFGS = {"dma_2": (2, 64, 2), "dma_3": (3, 64, 2), "dma_tall": (5, 64, 2), "dma_two": (6, 32, 3)}
# (M, N) of the two problems of a launch: one tile / two tiles of the 256-wide configurations, ragged in M or N
SHAPES = [((256, 256), (300, 256)), ((500, 256), (256, 260)), ((256, 512), (256, 256)), ((320, 256), (512, 252))]


def k_pairs(dkt):
    """Two different K per launch; together: 1 .. 5 stages, 72 and 200."""
    s = [dkt * i for i in range(1, 6)]
    return [(s[0], s[4]), (s[3], s[1]), (72, s[2]), (s[1], 200)]


def _cases():
    out = []
    for cfg, (_, dkt, _) in CFGS.items():
        for variant in (TN, NN):
            if cfg == "dma_tall" and variant == TN:
                continue                              # 320 rows are no whole 128-column sub-images: no k-strided X
            for i, ((k0, k1), (s0, s1)) in enumerate(zip(k_pairs(dkt), SHAPES)):
                xs = variant == TN and i == 1         # the bias column sums ride on one weight-gradient launch per configuration
                probs = [P(*s0, k0, colsum_a=xs), P(*s1, k1, accum=(i == 2), colsum_a=xs)]
                out.append(Case(f"ring/{cfg}/{G.VNAME[variant]}/K{k0}+{k1}" + ("/colsum_a" if xs else ""), cfg, BPM_BF16, variant, probs))
    # split-bf16 operands (automatic choice; it takes K >= 256 only, and weight gradients only from ~100 tiles up -- those
    # are table A's x3_2 row in test_gemm_groups_gpu.py -- so this is the NN form): 4 and 6 stages per plane pair, the last partial
    out.append(Case("ring/x3_3/NN/K256+328", "x3_3", BPM_F32, NN, [P(256, 256, 256), P(500, 256, 328)], x3=True))
    return out


CASES = _cases()


def stage_blocks(case, hs, dkt):
    """Add a constant per k stage to both operands (another one for every stage; exact in bf16) and renew the references'
    copies of the operands.  The pad columns stay zero."""
    xk, yk = case.variant != TN, False
    for h in hs:
        K = h.q.K
        stage = torch.arange(K) // dkt
        ca = 0.25 * (1 + stage).float()                       # 0.25, 0.5, ... per stage
        cb = 0.125 * (1 + (2 * stage) % 7).float()            # 0.125, 0.375, 0.625, 0.875, 0.25, ...
        for name, kcols, c, cols in (("A", xk, ca, h.L.a_cols), ("B", yk, cb, h.L.b_cols)):
            buf = getattr(h, name)
            v = buf[:, :cols].float()
            v = v + (c[None, :] if kcols else c[:, None])
            buf[:, :cols] = v.to(buf.dtype)
        h.Ar, h.Br = h.A[:, :h.L.a_cols].double(), h.B[:, :h.L.b_cols].double()


def _same_bits(a, b):
    return all(torch.equal(G._bits(x.C), G._bits(y.C)) and
               all((getattr(x, n) is None) or torch.equal(G._bits(getattr(x, n)), G._bits(getattr(y, n))) for n in ("colsum", "colsum_a"))
               for x, y in zip(a, b))


@pytest.mark.parametrize("case", CASES, ids=[c.id for c in CASES])
def test_ring_against_fp64(case):
    force, dkt, _ = CFGS.get(case.family_name, (-1, 64, 2))
    hs = G.make_host(case)
    stage_blocks(case, hs, dkt)
    ncu = torch.cuda.get_device_properties(0).multi_processor_count
    with _lib.lab_library() as L:
        _lib.check(L.bpm_debug_gemm_force(force), "bpm_debug_gemm_force")
        try:
            got, arr = G.launch(case, hs)
            again, _ = G.launch(case, hs)
        except RuntimeError as e:
            if "HIP error" in str(e) or "illegal memory access" in str(e):       # a faulted device runs nothing more in this session
                pytest.exit(f"{case.id}: GPU fault: {e}", returncode=3)
            raise
        out = (C.c_int * (4 + 4 * len(arr)))()
        rc = L.bpm_debug_gemm_choice(_lib.BPM_BF16X3 if case.x3 else case.dtype, case.variant, arr, len(arr), ncu, out)
    assert rc == 0 and G.KERNELS[out[0]] == case.family_name, f"{case.id}: ran as {G.KERNELS[out[0]]} (code {rc})"
    worst, fails, parts = G.check(case, hs, got)
    print(f"{case.id}: worst err / bound = {worst:.4g} {parts}")
    assert not fails, "\n".join(fails)
    assert worst <= 1.0
    assert _same_bits(got, again), f"{case.id}: two runs of the launch differ bitwise"


def test_cases_cover_the_ring():
    """The table holds what its docstring promises (no device needed for this, but it guards the GPU table)."""
    for cfg, (_, dkt, ns) in CFGS.items():
        for variant in (TN, NN):
            ks = {q.K for c in CASES if c.family_name == cfg and c.variant == variant for q in c.probs}
            if cfg == "dma_tall" and variant == TN:
                assert not ks
                continue
            assert {dkt * i for i in range(1, 6)} | {72, 200} <= ks and dkt * (ns + 1) in ks
        assert any(q.colsum_a for c in CASES if c.family_name == cfg for q in c.probs) or cfg == "dma_tall"
    for c in CASES:
        assert len(c.probs) == 2 and c.probs[0].K != c.probs[1].K and all(q.M <= 512 and q.N <= 512 for q in c.probs)
    assert any(c.x3 for c in CASES)
