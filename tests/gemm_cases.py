"""Grouped-GEMM launches of UNEQUAL problems for tests/test_gemm_groups_{cpu,gpu}.py (a plain helper module, not a conftest).

A `Case` is one bpm_gemm_grouped launch: compute type, operand arrangement and a list of problems `P(M, N, K, ...)`, every
problem with its own shape, leading dimensions, flags, output kind and side operands.  From a case this module builds

* the operands (CT-rounded, zero-padded rows as test_kernels_gpu.to_ct lays them out) and the output buffers with their
  GUARDS: at least one extra row behind row M, ldc > N for every fp32 / CT_NARROW output, guard cells pre-filled with a
  sentinel, the interior pre-filled with NaN where the kernel stores (with values where it adds).  After a launch every cell
  the kernel does not own must be bit-identical and the pad columns of a plain BPM_OUT_CT output exactly zero;
* the fp64 reference of the header's formula  v = ((acc + bias_n + bias_m) * alpha); ReLU; gate; dropout; + resid  on the
  rounded operands, with colsum (of the unrounded v, before the residual), colsum_a, ACCUM / ATOMIC (+= into the
  pre-filled values) and the head-major scatter; dropout multipliers are test_kernels_gpu.drop_mult (the hash restated);
* the bound, applied to EVERY element, s = max(1, max |ref|) of the problem's output:
      fp32 output, f32 or bf16 operands      |got - ref| <= 2e-5 s           (bf16 x bf16 products are exact in fp32 and the
                                                                             accumulators are fp32: the f32 mode's bound)
      bf16 CT / head-major output            |got - ref| <= 2^-8 |ref| + 2e-5 s    (the store's rounding of the element itself:
                                                                             round-to-nearest of an 8-bit significand comes to
                                                                             2^-8 at the bottom of a binade, so correct kernels
                                                                             sit just below 1; a truncating store does not pass)
      bf16x3                                 5e-5 s, against the fp32 operands
      colsum / colsum_a                      2e-5 max(1, sum over the column of |v|)
  and the dropout zero pattern, which must equal the hash's wherever |v| before dropout exceeds the absolute term;
* the problem structs, at device addresses (`launch`) or at made-up ones (`fake_structs`: the dispatcher's decision needs
  no device), and `family`: what bpm_debug_gemm_choice of the -DBPM_LAB build says the dispatcher does with them.

`emulate` is the fp32 CPU emulation of the documented arithmetic (fp32 matmul of the rounded operands, fp32 epilogue, bf16
rounding at the store) with optional injected defects: the no-GPU evidence that the reference alone stays inside the
bounds and that the bounds notice what they are meant to (tests/test_gemm_groups_cpu.py).

TABLE_A / TABLE_B / TABLE_C at the end are the launches both test files walk.
"""
import ctypes as C
from types import SimpleNamespace

import numpy as np
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, ops
from bpmult_amd._lib import (BPM_BF16, BPM_BF16X3, BPM_F32, F_ACCUM, F_ATOMIC, F_CT_NARROW, F_KPAD, F_RELU, GEMM_NN, GEMM_NT, GEMM_TN,
                             OUT_CT, OUT_F32, OUT_HEADS, GemmProblem)
from test_gemm_choice_cpu import KERNELS                      # enum Kernel of csrc/gemm.hip, by name
from test_kernels_gpu import drop_mult, host_key  # noqa: F401  (drop_mult keys the hash with host_key)

NT, NN, TN = GEMM_NT, GEMM_NN, GEMM_TN
VNAME = {NT: "NT", NN: "NN", TN: "TN"}
DNAME = {BPM_F32: "f32", BPM_BF16: "bf16"}
ABS_TERM = 2e-5                   # the project's tol(BPM_F32), relative to the largest element of the output
X3_TERM = 5e-5                    # the project's figure for the split-bf16 products
BF16_ULP = 2.0 ** -8              # half a bf16 ulp at the bottom of a binade: the most a round-to-nearest store moves an element
SENTINEL = -7744.0                # exact in bf16 and fp32; no reference value comes near it


def pad(n, to):
    return (n + to - 1) // to * to


def P(M, N, K, **kw):
    """One problem.  out: "f32" | "ct" | "narrow" (BPM_OUT_CT + CT_NARROW) | "heads" with heads = (B, H, dh, dhp), T = M / B.
    bias_n_off: elements the bias_n pointer sits behind a 16-byte boundary.  bias_m: "row" = [M], or ("elem", r): M = 1 and
    the pointer is element r of a longer bias (the pruned time maps).  gate = gate_scale.  tmap = Td: the TN time-map data
    gradient, A = rows {0, Td - 1} of W [Td, pad32(M)] through lda = (Td - 1) * ldw, K = 2.  dense_c: ldc = N exactly, as
    the engine lays its gradients out (table C only).  ones_b: B is the engine's vector of ones (bias gradients of the time
    maps).  kpad: override of the case's BPM_GEMM_KPAD_ZERO."""
    q = dict(M=M, N=N, K=K, bias_n=False, bias_n_off=0, bias_m=None, alpha=1.0, relu=False, gate=None, drop=0.0, site=0, resid=False,
             colsum=False, colsum_a=False, accum=False, atomic=False, splitk=1, out="f32", heads=None, ldc=None, ldr=None, tmap=None,
             dense_c=False, kpad=None, ones_b=False)
    assert not set(kw) - set(q), set(kw) - set(q)
    q.update(kw)
    return SimpleNamespace(**q)


class Case:
    def __init__(self, name, family, dtype, variant, probs, kpad=True, x3=False, seed=0x5EED):
        self.name, self.family_name, self.dtype, self.variant, self.probs = name, family, dtype, variant, probs
        self.kpad, self.x3, self.seed = kpad, x3, seed
        assert not x3 or dtype == BPM_F32

    @property
    def id(self):
        return f"{self.name}-{'x3' if self.x3 else DNAME[self.dtype]}"

    def shapes_differ(self):
        return len({(q.M, q.N, q.K) for q in self.probs}) > 1

    def features(self, q):
        """The epilogue features of a problem, as the engine-signature test names them."""
        f = {k for k in ("bias_n", "relu", "resid", "colsum", "colsum_a", "accum", "atomic") if getattr(q, k)}
        f |= {"bias_m"} if q.bias_m else set()
        f |= {"alpha"} if q.alpha != 1.0 else set()
        f |= {"gate"} if q.gate is not None else set()
        f |= {"drop"} if q.drop > 0 else set()
        f |= {"splitk"} if q.splitk > 1 else set()
        f |= {"out_" + ("ct" if q.out == "narrow" else q.out)} | ({"narrow"} if q.out == "narrow" else set())
        return f


# ---------------------------------------------------------------------------
# layout: leading dimensions and buffer sizes of one problem (no data)
# ---------------------------------------------------------------------------
def layout(case, q):
    xk, yk = case.variant != TN, case.variant == NT
    L = SimpleNamespace()
    L.a_rows, L.a_cols = (q.M, q.K) if xk else (q.K, q.M)
    L.b_rows, L.b_cols = (q.N, q.K) if yk else (q.K, q.N)
    # k-contiguous rows hold whole 64-element stages (what the LDS-DMA kernel asks for), k-strided rows 32-element pads
    L.lda = pad(L.a_cols, 64 if xk else 32)
    L.ldb = pad(L.b_cols, 64 if yk else 32)
    L.a_alloc = (L.a_rows, L.lda)
    if q.tmap:                                        # A = W [Td, ldw]; the two k rows are Td - 1 rows apart
        assert case.variant == TN and q.K == 2
        L.a_alloc = (q.tmap, L.lda)
        L.lda = (q.tmap - 1) * L.lda
    L.out_f32 = q.out == "f32" or case.dtype == BPM_F32           # element type of the output buffer (bf16x3: fp32 CT)
    L.ldg = pad(q.N, 32)
    L.ldr = q.ldr or q.N + 4
    if q.out == "heads":
        B, H, dh, dhp = q.heads
        assert q.M % B == 0 and H * dh == q.N and dhp >= dh
        L.T = q.M // B
        L.ldc = 0
        L.c_elems = B * H * L.T * dhp + dhp                       # one guard row of dhp elements behind the last head row
    else:
        L.ldc = q.ldc or (q.N if q.dense_c else q.N + 4 if q.out == "f32" else pad(q.N, 32) + (32 if q.out == "narrow" else 0))
        assert q.dense_c or q.out == "ct" or L.ldc > q.N
        L.c_elems = (q.M + 1) * L.ldc                             # one guard row behind row M
    L.plain = not (q.accum or q.atomic)
    return L


def flags_of(case, q):
    kp = case.kpad if q.kpad is None else q.kpad
    return ((F_KPAD if kp else 0) | (F_ACCUM if q.accum else 0) | (F_ATOMIC if q.atomic else 0) | (F_RELU if q.relu else 0) |
            (F_CT_NARROW if q.out == "narrow" else 0))


def structs(case, addr):
    """The launch's problem array.  addr(i, name) -> address of buffer `name` of problem i (its first element)."""
    out = []
    for i, q in enumerate(case.probs):
        L = layout(case, q)
        p = GemmProblem()
        p.A, p.B, p.C = addr(i, "A"), addr(i, "B"), addr(i, "C")
        p.M, p.N, p.K = q.M, q.N, q.K
        p.lda, p.ldb, p.ldc = L.lda, L.ldb, L.ldc
        if q.bias_n:
            p.bias_n = addr(i, "bias_n") + 4 * q.bias_n_off
        if q.bias_m:
            p.bias_m = addr(i, "bias_m") + (4 * q.bias_m[1] if q.bias_m != "row" else 0)
        if q.resid:
            p.resid, p.ldr = addr(i, "resid"), L.ldr
        if q.gate is not None:
            p.gate, p.ldg, p.gate_scale = addr(i, "gate"), L.ldg, q.gate
        else:
            p.gate_scale = 1.0
        p.alpha, p.drop_p, p.drop_site = q.alpha, q.drop, q.site
        if q.colsum:
            p.colsum = addr(i, "colsum")
        if q.colsum_a:
            p.colsum_a = addr(i, "colsum_a")
        p.flags, p.splitk = flags_of(case, q), q.splitk
        p.out_kind = {"f32": OUT_F32, "ct": OUT_CT, "narrow": OUT_CT, "heads": OUT_HEADS}[q.out]
        if q.out == "heads":
            B, H, dh, dhp = q.heads
            p.heads_B, p.heads_H, p.heads_T, p.heads_dh, p.heads_dhp = B, H, L.T, dh, dhp
        out.append(p)
    return ops.array(GemmProblem, out)


def fake_structs(case):
    """The same array at made-up (never read) addresses, 256-byte aligned as the caching allocator's are."""
    table = {}

    def addr(i, name):
        return table.setdefault((i, name), 0x7F0000000000 + (len(table) << 28))
    arr = structs(case, addr)
    return x3_structs(arr, case.variant) if case.x3 else arr


def x3_structs(arr, variant):
    """What ops._X3Plan sends for an fp32 launch in bf16x3 mode: split images [rows, hi plane | lo plane], planes padded to
    128 columns (the images sit at the fp32 operands' made-up addresses: the choice never reads them)."""
    xk, yk = variant != TN, variant == NT
    out = []
    for p in arr:
        assert ops._X3Plan._eligible(p), "the split path would leave this problem to the exact fp32 kernels"
        q = GemmProblem()
        C.memmove(C.byref(q), C.byref(p), C.sizeof(GemmProblem))
        q.lda, q.ldb = 2 * pad(p.K if xk else p.M, 128), 2 * pad(p.K if yk else p.N, 128)
        q.flags |= F_KPAD
        out.append(q)
    return ops.array(GemmProblem, out)


def family(case, ncu, arr=None):
    """(kernel family, [(tile0, tiles_m, tiles_n, splitk) per problem], total tiles): bpm_debug_gemm_choice of the lab build
    on the launch's real problem array (`arr`; default: the made-up addresses).  Raises HipLibraryError without that build."""
    arr = fake_structs(case) if arr is None else arr
    n = len(arr)
    out = (C.c_int * (4 + 4 * n))()
    with _lib.lab_library() as L:
        rc = L.bpm_debug_gemm_choice(BPM_BF16X3 if case.x3 else case.dtype, case.variant, arr, n, ncu, out)
    assert rc == 0, f"{case.id}: the dispatcher rejects the launch with code {rc}"
    return KERNELS[out[0]], [tuple(out[4 + 4 * i:8 + 4 * i]) for i in range(n)], out[3]


# ---------------------------------------------------------------------------
# host data, fp64 reference, fp32 emulation
# ---------------------------------------------------------------------------
def make_host(case):
    """Per problem: every buffer of the launch as a CPU tensor (the outputs in their initial state), plus the index maps of
    the cells the kernel owns."""
    ctt = ops.ct_torch(case.dtype)
    hs = []
    for i, q in enumerate(case.probs):
        L = layout(case, q)
        g = torch.Generator().manual_seed(case.seed * 1009 + i)
        rnd = lambda *shape, scale=1.0: torch.randn(*shape, generator=g) * scale

        def ctbuf(rows, cols, ld, scale=1.0):
            buf = torch.zeros(rows, ld, dtype=ctt)
            buf[:, :cols] = rnd(rows, cols, scale=scale).to(ctt)
            return buf
        h = SimpleNamespace(L=L, q=q)
        if q.tmap:
            W = ctbuf(q.tmap, q.M, L.a_alloc[1])
            h.A, h.Ar = W, W[[0, q.tmap - 1], :q.M].double()
        else:
            # (a product against ones keeps its terms at K^-1/2 like every other problem's: the bounds are relative to an
            #  output of order one, not to partial sums of order K^1/2)
            h.A = ctbuf(L.a_rows, L.a_cols, L.lda, scale=q.K ** -0.5 if q.ones_b else 1.0)
            h.Ar = h.A[:, :L.a_cols].double()
        h.B = ctbuf(L.b_rows, L.b_cols, L.ldb, scale=q.K ** -0.5)
        if q.ones_b:
            h.B[:, :L.b_cols] = 1
        h.Br = h.B[:, :L.b_cols].double()
        if q.bias_n:
            h.bias_n = rnd(q.bias_n_off + q.N)
        if q.bias_m:
            h.bias_m = rnd(q.M if q.bias_m == "row" else q.bias_m[1] + 1)
        if q.resid:
            h.resid = rnd(q.M, L.ldr)
        if q.gate is not None:
            h.gate = ctbuf(q.M, q.N, L.ldg)
        if q.colsum:
            h.colsum = torch.cat([rnd(q.N), torch.full((4,), SENTINEL)])
        if q.colsum_a:
            h.colsum_a = torch.cat([rnd(q.M), torch.full((4,), SENTINEL)])
        h.dm = drop_mult((q.M, q.N), q.drop, case.seed, q.site).double() if q.drop > 0 else None
        # the output buffer: sentinel everywhere, then NaN (stores) or values (+=) in the cells the kernel owns
        m, n = torch.meshgrid(torch.arange(q.M), torch.arange(q.N), indexing="ij")
        if q.out == "heads":
            B, H, dh, dhp = q.heads
            h.idx = (((m % B) * H + n // dh) * L.T + m // B) * dhp + n % dh
            h.zero_idx = torch.zeros(0, dtype=torch.long)
        else:
            h.idx = m * L.ldc + n
            mz, nz = torch.meshgrid(torch.arange(q.M), torch.arange(q.N, L.ldc), indexing="ij")
            h.zero_idx = (mz * L.ldc + nz).reshape(-1) if q.out == "ct" else torch.zeros(0, dtype=torch.long)
        assert h.idx.unique().numel() == q.M * q.N
        c = torch.full((L.c_elems,), SENTINEL)
        c[h.idx.reshape(-1)] = float("nan") if L.plain else rnd(q.M * q.N)
        h.C = c if L.out_f32 else c.to(torch.bfloat16)
        h.owned = torch.zeros(L.c_elems, dtype=torch.bool)
        h.owned[h.idx.reshape(-1)] = True
        h.owned[h.zero_idx] = True
        hs.append(h)
    return hs


def _bf16(x):
    return x.to(torch.bfloat16).to(x.dtype)


def evaluate(case, h, dt, defect=None, nxt=None):
    """The header's formula in precision dt.  -> out [M, N] (before the store's rounding), v (before the residual),
    pre = |v| before dropout, colsum [N], colsum_a [M].  `defect`: see emulate()."""
    q = h.q
    A, B = h.Ar.to(dt), h.Br.to(dt)
    mm = {NT: lambda a, b: a @ b.T, NN: lambda a, b: a @ b, TN: lambda a, b: a.T @ b}[case.variant]
    acc = mm(A, B)
    kdim = 0 if case.variant == TN else 1
    if defect == "last k of a row dropped":
        r = q.M // 2
        last = (A[-1, r] * B[-1, :]) if case.variant == TN else (A[r, -1] * (B[:, -1] if case.variant == NT else B[-1, :]))
        acc[r] = acc[r] - last
    if defect == "accumulator rounded to bf16 in mid-sum":
        k2 = A.shape[kdim] // 2
        sl = (lambda x, lo, hi: x[lo:hi]) if case.variant == TN else (lambda x, lo, hi: x[:, lo:hi])
        slb = (lambda x, lo, hi: x[:, lo:hi]) if case.variant == NT else (lambda x, lo, hi: x[lo:hi])
        acc = _bf16(mm(sl(A, 0, k2), slb(B, 0, k2))) + mm(sl(A, k2, None), slb(B, k2, None))
    if defect == "bias added after a bf16 rounding":
        acc = _bf16(acc)
    v = acc
    if q.bias_n:
        v = v + h.bias_n[q.bias_n_off:].to(dt)[None, :]
    if q.bias_m:
        v = v + (h.bias_m if q.bias_m == "row" else h.bias_m[q.bias_m[1]:]).to(dt)[:, None]
    v = v * float(np.float32(q.alpha))
    if q.relu:
        v = v.clamp(min=0)
    if q.gate is not None:
        v = torch.where(h.gate[:, :q.N].to(dt) > 0, v * float(np.float32(q.gate)), torch.zeros((), dtype=dt))
    pre = v.abs()
    if h.dm is not None:
        dm = h.dm
        if defect == "dropout index of a row shifted by one":
            dm = dm.clone()
            r = q.M // 2
            dm[r] = torch.roll(h.dm.reshape(-1), -1)[r * q.N:(r + 1) * q.N]
        v = v * dm.to(dt)
    colsum = v.sum(0)
    if defect == "last row missing from colsum":
        colsum = v[:-1].sum(0)
    out = v
    if q.resid:
        out = out + h.resid[:, :q.N].to(dt)
    if not h.L.plain:
        out = out + h.C[h.idx].to(dt)
    if defect == "a 16 x 16 tile from the next problem" and nxt is not None:
        out = out.clone()
        out[:16, :16] = nxt[:16, :16]
    return SimpleNamespace(out=out, v=v, pre=pre, colsum=colsum, colsum_a=A.sum(0) if q.colsum_a else None)


DEFECTS = {  # name -> the problem of the launch it is injected into must have ...
    "last k of a row dropped": lambda q: q.out == "f32",
    "bias added after a bf16 rounding": lambda q: q.out == "f32" and q.bias_n,
    "accumulator rounded to bf16 in mid-sum": lambda q: q.out == "f32",
    "a 16 x 16 tile from the next problem": lambda q: True,
    "dropout index of a row shifted by one": lambda q: q.drop > 0,
    "last row missing from colsum": lambda q: q.colsum,
    "a guard cell written": lambda q: True,
    "a pad column of a CT output non-zero": lambda q: q.out == "ct" and q.N % 32 != 0,
}


def emulate(case, hs, defect=None):
    """What a correct kernel leaves in the buffers, by fp32 CPU arithmetic: fp32 matmul of the rounded operands, the
    epilogue in fp32, bf16 rounding at the store.  defect (a key of DEFECTS): injected into the first problem that has
    what the defect needs.  -> the `got` list check() takes."""
    assert not case.x3, "the emulation restates the f32 / bf16 kernels"
    target = None if defect is None else next(i for i, h in enumerate(hs) if DEFECTS[defect](h.q))
    clean = [evaluate(case, h, torch.float32) for h in hs]
    got = []
    for i, h in enumerate(hs):
        e = clean[i]
        if i == target:
            e = evaluate(case, h, torch.float32, defect, clean[(i + 1) % len(hs)].out)
        c = h.C.clone()
        c[h.idx.reshape(-1)] = e.out.reshape(-1).to(c.dtype)
        c[h.zero_idx] = 0
        if i == target and defect == "a guard cell written":
            c[int((~h.owned).nonzero()[0])] = 1.0
        if i == target and defect == "a pad column of a CT output non-zero":
            c[h.zero_idx[len(h.zero_idx) // 2]] = 2.0 ** -20
        r = SimpleNamespace(C=c, colsum=None, colsum_a=None)
        if h.q.colsum:
            r.colsum = h.colsum.clone()
            r.colsum[:h.q.N] += e.colsum
        if h.q.colsum_a:
            r.colsum_a = h.colsum_a.clone()
            r.colsum_a[:h.q.M] += e.colsum_a
        got.append(r)
    return got


def _bits(t):
    return t.view(torch.int32 if t.dtype == torch.float32 else torch.int16)


def check(case, hs, got):
    """-> (worst err / bound of the case, [failure messages], the worst ratio per kind of figure: fp32 outputs, bf16 outputs,
    column sums).  Every element of every output is held to its bound."""
    worst, fails, parts = 0.0, [], {}
    for i, (h, r) in enumerate(zip(hs, got)):
        q, tag = h.q, f"{case.id} problem {i} ({h.q.M} x {h.q.N} x {h.q.K}, {h.q.out})"
        ref = evaluate(case, h, torch.float64)
        c = r.C.cpu()
        assert c.dtype == h.C.dtype and c.shape == h.C.shape
        if not torch.equal(_bits(c)[~h.owned], _bits(h.C)[~h.owned]):
            bad = ((_bits(c) != _bits(h.C)) & ~h.owned).nonzero().reshape(-1)
            fails.append(f"{tag}: {bad.numel()} guard cells written, first at element {int(bad[0])} (ldc {h.L.ldc})")
        if h.zero_idx.numel() and not bool((c[h.zero_idx] == 0).all()):
            fails.append(f"{tag}: pad columns [N, ldc) of a BPM_OUT_CT output must be exactly zero")
        val = c[h.idx].double()
        s = max(1.0, ref.out.abs().max().item())
        term = (X3_TERM if case.x3 else ABS_TERM) * s
        bound = torch.full_like(ref.out, term)
        if not h.L.out_f32:
            bound = bound + BF16_ULP * ref.out.abs()
        if not bool(torch.isfinite(val).all()):
            fails.append(f"{tag}: {int((~torch.isfinite(val)).sum())} elements not written or not finite")
            worst = float("inf")
        else:
            ratio = ((val - ref.out).abs() / bound).max().item()
            worst = max(worst, ratio)
            kind = "fp32_out" if h.L.out_f32 else "bf16_out"
            parts[kind] = max(parts.get(kind, 0.0), ratio)
            if ratio > 1:
                m, n = np.unravel_index(int(((val - ref.out).abs() / bound).argmax()), ref.out.shape)
                fails.append(f"{tag}: err / bound = {ratio:.3g} at ({m}, {n}): got {val[m, n]:.9g}, fp64 {ref.out[m, n]:.9g}, bound {bound[m, n]:.3g}")
            if h.dm is not None and not q.resid and h.L.plain:
                sure = ref.pre > term
                if not torch.equal((val == 0)[sure], (h.dm == 0)[sure]):
                    fails.append(f"{tag}: the dropout zero pattern differs from the hash's in {int(((val == 0) != (h.dm == 0))[sure].sum())} elements")
        for name, n, refsum, mass in (("colsum", q.N, ref.colsum, ref.v.abs().sum(0)), ("colsum_a", q.M, ref.colsum_a, h.Ar.abs().sum(0))):
            if not getattr(q, name):
                continue
            init, out = getattr(h, name), getattr(r, name).cpu()
            if not torch.equal(_bits(out)[n:], _bits(init)[n:]):
                fails.append(f"{tag}: {name} written past its {n} elements")
            bnd = ABS_TERM * mass.clamp(min=1.0)
            ratio = ((out[:n].double() - init[:n].double() - refsum).abs() / bnd).max().item()
            ratio = ratio if np.isfinite(ratio) else float("inf")
            worst = max(worst, ratio)
            parts["colsum"] = max(parts.get("colsum", 0.0), ratio)
            if not ratio <= 1:
                fails.append(f"{tag}: {name} err / bound = {ratio:.3g}")
    return worst, fails, parts


# ---------------------------------------------------------------------------
# the launch (product library)
# ---------------------------------------------------------------------------
def launch(case, hs):
    """Run the case through ops.gemm_grouped (the PRODUCT library).  -> (got, the problem array the library saw).  Every
    device tensor stays alive until the results are back: the problems hold raw pointers."""
    names = ("A", "B", "C", "bias_n", "bias_m", "resid", "gate", "colsum", "colsum_a")
    dev = [{n: getattr(h, n).cuda() for n in names if hasattr(h, n)} for h in hs]
    arr = structs(case, lambda i, name: dev[i][name].data_ptr())
    ops.gemm_grouped(case.dtype, case.variant, arr, seed=case.seed, x3=ops.X3Cache(torch.device("cuda")) if case.x3 else None)
    torch.cuda.synchronize()
    got = [SimpleNamespace(C=d["C"].cpu(), colsum=d["colsum"].cpu() if "colsum" in d else None,
                           colsum_a=d["colsum_a"].cpu() if "colsum_a" in d else None) for d in dev]
    seen = arr
    if case.x3:
        plan = arr._x3_plan
        assert plan.ok and plan.rest is None, "every problem of a bf16x3 row must run as split-bf16 products"
        seen = plan.gemm
    del dev
    return got, seen


# ---------------------------------------------------------------------------
# the tables.  Shapes: the smallest the rules of choose() / summarise() in csrc/gemm.hip still send to the family at 256
# compute units (tests/test_gemm_groups_cpu.py asks the dispatcher).  Every multi-problem row: no two problems of one
# shape, one ragged in M, one ragged in N with N % 4 == 0, one whose K is no whole k stage, one single tile, the first
# and the last problem the smallest.
# ---------------------------------------------------------------------------
def _epi(k, variant, shape, site):
    """Epilogue k of the LDS-DMA rows (the 4-wide epilogue only: GroupShape::legal)."""
    M, N, K = shape
    if k == "plain":
        return P(M, N, K)
    if k == "bias_resid":
        return P(M, N, K, bias_n=True, resid=True)
    if k == "drop_resid":                             # residual dropout of the attention / FFN output projections
        return P(M, N, K, bias_n=True, drop=0.1, site=site, resid=True)
    if k == "relu_drop_ct":
        return P(M, N, K, bias_n=True, relu=True, drop=0.3, site=site, out="ct")
    if k == "gate_colsum_ct":
        return P(M, N, K, gate=1.25, colsum=True, out="ct")
    if k == "accum":
        return P(M, N, K, accum=True)
    if k == "colsum_a":
        return P(M, N, K, colsum_a=True)
    if k == "accum_colsum_a":
        return P(M, N, K, accum=True, colsum_a=True)
    if k == "narrow":
        return P(M, N, K, bias_n=True, out="narrow")
    if k.startswith("heads") or k.startswith("pheads"):       # heads<dh>: bias + alpha + head-major scatter; pheads<dh>: the scatter alone
        dh = int(k.lstrip("pheads"))
        B = 8 if M % 8 == 0 else 4
        assert N % dh == 0 and M % B == 0, (k, shape)
        side = dict(bias_n=True, alpha=0.2) if k.startswith("heads") else {}
        return P(M, N, K, out="heads", heads=(B, N // dh, dh, pad(dh, 32)), **side)
    raise KeyError(k)


def _row(variant, items):
    return [_epi(k, variant, shape, 3 + i) for i, (shape, k) in enumerate(items)]


# 256 x 256 tiles: every problem fills them to 80 %; N = 420 = 6 heads of 70 (dh % 4 != 0), 448 = 7 heads of 64
_BIG_NT = [((256, 256, 256), "plain"), ((420, 256, 264), "bias_resid"), ((256, 440, 320), "relu_drop_ct"), ((512, 512, 330), "gate_colsum_ct"),
           ((500, 448, 256), "accum"), ((256, 448, 288), "heads64"), ((256, 420, 256), "heads70"), ((440, 256, 288), "drop_resid"),
           ((256, 256, 288), "narrow")]
_BIG_NN = [((256, 256, 256), "plain"), ((420, 256, 264), "bias_resid"), ((256, 440, 320), "relu_drop_ct"), ((512, 512, 330), "gate_colsum_ct"),
           ((500, 448, 256), "accum"), ((256, 448, 288), "pheads64"), ((440, 256, 288), "drop_resid"), ((256, 256, 288), "narrow")]
# 320 x 256 tiles save a round when the 256-row tiles need two: M = 640 is 3 against 2 tiles per column block
_TALL = [((256, 256, 256), "plain"), ((640, 4096, 256), "bias_resid"), ((630, 4096, 264), "relu_drop_ct"), ((640, 4092, 320), "gate_colsum_ct"),
         ((640, 4096, 288), "accum"), ((640, 3840, 330), "pheads64"), ((640, 1792, 256), "narrow"), ((256, 256, 288), "bias_resid")]
_TALL_NT = _TALL[:-1] + [((640, 1792, 264), "heads64"), ((640, 1000, 320), "heads50"),
                         ((256, 256, 1088), "drop_resid")]     # K > 1024 keeps the N >= 2048 two-resident rule off
_TWELVE = _BIG_NT[:-2] + [((512, 256, 256), "plain"), ((256, 512, 264), "bias_resid"), ((500, 512, 320), "accum"), ((440, 256, 330), "relu_drop_ct"),
                          ((256, 256, 288), "narrow")]
_WIDE = [((256, 256, 256), "plain"), ((256, 2048, 264), "bias_resid"), ((420, 2044, 320), "relu_drop_ct"), ((512, 512, 330), "gate_colsum_ct"),
         ((256, 448, 288), "heads64"), ((256, 420, 256), "heads70"), ((256, 256, 288), "accum")]
# narrow rule: 256 x 128 tiles filled to 75 %, at least one per CU; N = 300 = 5 heads of 60 = 6 of 50, 128 = 2 heads of 64
_NARROW = [((256, 128, 256), "plain"), ((4000, 300, 300), "bias_resid"), ((3000, 300, 264), "relu_drop_ct"), ((4090, 300, 330), "gate_colsum_ct"),
           ((4050, 300, 288), "accum"), ((2040, 300, 320), "narrow"), ((4000, 300, 264), "plain"), ((1000, 300, 256), "bias_resid"),
           ((500, 300, 320), "accum")]
_NARROW_NT = _NARROW + [((4000, 300, 320), "heads50"), ((256, 128, 288), "heads64")]
_NARROW_NN = _NARROW + [((4000, 300, 320), "gate_colsum_ct"), ((256, 128, 288), "bias_resid")]
# weight gradients on the LDS-DMA kernel: 160 tiles of 256 x 256 at 256 compute units
_TN_TWO = [((256, 256, 1024), "plain"), ((1024, 2048, 1024), "accum"), ((1024, 2048, 1030), "bias_resid"), ((1024, 2048, 1088), "plain"),
           ((1024, 2048, 1100), "accum"), ((1000, 1024, 1024), "plain"), ((1024, 1000, 1056), "accum"), ((256, 256, 1030), "accum")]
_TN_2 = [((256, 256, 256), "colsum_a"), ((1024, 2048, 256), "accum"), ((1024, 2048, 264), "accum_colsum_a"), ((1024, 2048, 320), "plain"),
         ((1024, 2048, 330), "colsum_a"), ((1000, 1024, 256), "accum_colsum_a"), ((1024, 1000, 288), "bias_resid"), ((256, 256, 264), "accum")]

# the register-staged kernels: problems too small for the LDS-DMA tiles
_SMALL = [((40, 64, 24), "plain"), ((300, 140, 200), "bias_resid"), ((129, 68, 330), "relu_drop_ct"), ((200, 100, 64), "gate_colsum_ct"),
          ((128, 64, 100), "accum"), ((70, 128, 96), "narrow"), ((88, 128, 40), "pheads64"), ((50, 64, 40), "bias_resid")]
_SMALL_NT = _SMALL[:-1] + [((80, 128, 72), "heads64"), ((120, 100, 256), "heads25"), ((50, 64, 40), "drop_resid")]
_SKINNY = [((1, 64, 32), "plain"), ((16, 140, 200), "bias_resid"), ((13, 68, 330), "relu_drop_ct"), ((8, 100, 64), "gate_colsum_ct"),
           ((15, 200, 100), "accum"), ((5, 64, 96), "narrow"), ((3, 200, 264), "plain"), ((8, 64, 40), "pheads64"), ((2, 64, 40), "bias_resid")]
_SKINNY_NT = _SKINNY[:-1] + [((16, 128, 72), "heads64"), ((12, 100, 256), "heads25"), ((2, 64, 40), "drop_resid")]


def _tn(items):
    """Weight-gradient rows of the register-staged kernels: (shape, ACCUM | colsum_a | ATOMIC with splitk)."""
    out = []
    for (M, N, K), k in items:
        if k.startswith("atomic"):
            out.append(P(M, N, K, atomic=True, splitk=int(k[6:])))
        else:
            out.append(_epi(k, TN, (M, N, K), 0))
    return out


_TN_SMALL = [((64, 64, 40), "plain"), ((300, 140, 1000), "atomic3"), ((129, 68, 330), "colsum_a"), ((200, 100, 64), "atomic1"),
             ((128, 64, 100), "accum"), ((70, 130, 96), "accum_colsum_a"), ((50, 64, 24), "atomic1")]
# 512 workgroups of 128 x 64 (split-K slices counted) send hardware-bounded weight gradients to the 128-row kernel
_TN_MANY = [((64, 64, 40), "plain"), ((1024, 1024, 64), "accum"), ((1000, 1024, 70), "colsum_a"), ((1024, 1000, 33), "atomic1"),
            ((512, 512, 100), "atomic3"), ((1024, 960, 48), "accum_colsum_a"), ((128, 64, 24), "atomic1")]


def _table_a():
    BF, F32 = BPM_BF16, BPM_F32
    rows = [
        Case("A/dma_3/NT", "dma_3", BF, NT, _row(NT, _BIG_NT)),
        Case("A/dma_3/NN", "dma_3", BF, NN, _row(NN, _BIG_NN)),
        Case("A/dma_tall/NT", "dma_tall", BF, NT, _row(NT, _TALL_NT)),
        Case("A/dma_tall/NN", "dma_tall", BF, NN, _row(NN, _TALL)),
        Case("A/dma_two/NT/twelve", "dma_two", BF, NT, _row(NT, _TWELVE)),
        Case("A/dma_two/NT/wide", "dma_two", BF, NT, _row(NT, _WIDE)),
        Case("A/dma_two/NT/narrow", "dma_two", BF, NT, _row(NT, _NARROW_NT)),
        Case("A/dma_two/NN/narrow", "dma_two", BF, NN, _row(NN, _NARROW_NN)),
        Case("A/dma_two/TN", "dma_two", BF, TN, _row(TN, _TN_TWO)),
        Case("A/dma_2/TN", "dma_2", BF, TN, _row(TN, _TN_2)),
        Case("A/x3_3/NT", "x3_3", F32, NT, _row(NT, _BIG_NT), x3=True),
        Case("A/x3_3/NN", "x3_3", F32, NN, _row(NN, _BIG_NN), x3=True),
        Case("A/x3_tall/NN", "x3_tall", F32, NN, _row(NN, _TALL), x3=True),
        Case("A/x3_2/TN", "x3_2", F32, TN, _row(TN, _TN_2), x3=True),
    ]
    for dt in (BF, F32):
        rows += [
            Case("A/skinny/NT", "skinny", dt, NT, _row(NT, _SKINNY_NT)),
            Case("A/skinny/NN", "skinny", dt, NN, _row(NN, _SKINNY)),
            Case("A/tiled_fast/NT", "tiled_fast", dt, NT, _row(NT, _SMALL_NT)),
            Case("A/tiled_fast/NN", "tiled_fast", dt, NN, _row(NN, _SMALL)),
            Case("A/tiled_fast/TN", "tiled_fast", dt, TN, _tn(_TN_MANY)),
            Case("A/tiled_bounded/NT", "tiled_bounded", dt, NT, _row(NT, _SMALL_NT), kpad=False),
            Case("A/tiled_bounded/NN", "tiled_bounded", dt, NN, _row(NN, _SMALL), kpad=False),
            Case("A/tn_64/TN", "tn_64", dt, TN, _tn(_TN_SMALL)),
            Case("A/tn_short/TN", "tn_short", dt, TN, _tn(_TN_MANY), kpad=False),
            Case("A/tn_long/TN", "tn_long", dt, TN, _tn(_TN_SMALL), kpad=False),
        ]
    return rows


# (family, variant) pairs table A must contain
TABLE_A_PAIRS = {("dma_3", NT), ("dma_3", NN), ("dma_tall", NT), ("dma_tall", NN), ("dma_two", NT), ("dma_two", NN), ("dma_two", TN),
                 ("dma_2", TN), ("x3_3", NT), ("x3_tall", NN), ("x3_2", TN), ("skinny", NT), ("skinny", NN), ("tiled_fast", NT),
                 ("tiled_fast", NN), ("tiled_fast", TN), ("tiled_bounded", NT), ("tiled_bounded", NN), ("tn_64", TN), ("tn_short", TN),
                 ("tn_long", TN)}


def _general(rows16):
    """Table B: problems epi_fast_ok refuses -- N % 4 != 0, ldc % 4 != 0, a bias_n pointer off 16 bytes, bias_m,
    resid + ACCUM -- each with one of the epilogues no kernel test sent through the general epilogue, beside fast-epilogue
    problems in the same grid.  rows16: shapes for the skinny kernel (at most 16 rows)."""
    S = (lambda big, small: small) if rows16 else (lambda big, small: big)
    return [
        P(S(40, 2), 64, 24, bias_n=True, resid=True),                                          # fast epilogue; single tile
        P(S(200, 16), 72, 100, bias_m="row"),                                                   # bias_m alone
        P(S(129, 13), 70, 330, bias_m="row", bias_n=True),                                      # ... with bias_n; N % 4 != 0
        P(S(300, 15), 140, 200, alpha=0.3, ldc=143),                                            # ldc % 4 != 0; N ragged, N % 4 == 0
        P(S(130, 9), 96, 64, bias_n=True, bias_n_off=1, relu=True, drop=0.3, site=7, out="ct"),  # bias_n off 16 bytes
        P(S(150, 11), 65, 96, gate=1.25, colsum=True, out="ct"),                                # N % 4 != 0
        P(S(120, 10), 75, 40, bias_n=True, alpha=0.2, out="heads", heads=(S(5, 2), 3, 25, 32)),   # dh = 25
        P(S(140, 7), 68, 72, resid=True, accum=True),                                           # resid + ACCUM
        P(S(131, 5), 77, 264, drop=0.25, site=9),                                               # dropout -> fp32, hash index not quad aligned
        P(S(100, 16), 128, 48, gate=0.5, colsum=True, bias_n=True, out="narrow"),                # fast epilogue
        P(S(50, 1), 64, 40, bias_m="row", accum=True),                                          # single tile
    ]


def _table_b():
    rows = []
    for dt in (BPM_BF16, BPM_F32):
        for v in (NT, NN):
            rows += [Case(f"B/tiled_fast/{VNAME[v]}", "tiled_fast", dt, v, _general(False)),
                     Case(f"B/tiled_bounded/{VNAME[v]}", "tiled_bounded", dt, v, _general(False), kpad=False),
                     Case(f"B/skinny/{VNAME[v]}", "skinny", dt, v, _general(True))]
    return rows


TMAPS = [(20, 50), (50, 33), (33, 20)]                # (Ts, Td) of the maps of one launch


def _table_c():
    """The time-axis Linear maps as models/bpmult.py::_build_time issues them (no F_KPAD, dense fp32 gradients: ldc = N;
    the two single-row products of a pruned map have one shape, as in the engine).  The products against the vector of
    ones draw their other operand at K^-1/2 (make_host) so that, as everywhere in these tables, the terms of a sum have the
    size of the bound's scale: with terms of order one the f32 mode's K = 6144 sum (one accumulator, 1536 serial MFMA steps,
    partial sums near 80) measured 4.5e-5 from fp64 at an output of 0.21 -- fp32 accumulation, 2.2 x the bound at s = 1."""
    rows = []
    for dt in (BPM_BF16, BPM_F32):
        for BD, tag in ((2 * 40, "2x40"), (8 * 768, "8x768")):
            fwd, wg, dg, dfwd, dwg, ddg = [], [], [], [], [], []
            for Ts, Td in TMAPS:
                for r in (0, Td - 1):
                    fwd.append(P(1, BD, Ts, bias_m=("elem", r), dense_c=True))
                    wg.append(P(1, Ts, BD, accum=True, dense_c=True))
                    wg.append(P(1, 1, BD, accum=True, dense_c=True, ones_b=True))
                dg.append(P(Ts, BD, 2, tmap=Td, dense_c=True))
                dfwd.append(P(Td, BD, Ts, bias_m="row", dense_c=True))
                dwg.append(P(Td, Ts, BD, accum=True, dense_c=True))
                dwg.append(P(Td, 1, BD, accum=True, dense_c=True, ones_b=True))
                ddg.append(P(Ts, BD, Td, dense_c=True))
            rows += [Case(f"C/pruned/forward/{tag}", "tiled_bounded", dt, NN, fwd, kpad=False),
                     Case(f"C/pruned/weight-grad/{tag}", "tiled_bounded", dt, NT, wg, kpad=False),
                     Case(f"C/pruned/data-grad/{tag}", "tn_long", dt, TN, dg, kpad=False),
                     Case(f"C/dense/forward/{tag}", "tiled_bounded", dt, NN, dfwd, kpad=False),
                     Case(f"C/dense/weight-grad/{tag}", "tiled_bounded", dt, NT, dwg, kpad=False),
                     Case(f"C/dense/data-grad/{tag}", "tn_long", dt, TN, ddg, kpad=False)]
    return rows


TABLE_A, TABLE_B, TABLE_C = _table_a(), _table_b(), _table_c()
TABLES = TABLE_A + TABLE_B + TABLE_C
