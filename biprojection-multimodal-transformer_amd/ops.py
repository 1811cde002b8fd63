"""Thin Python wrappers over the C ABI (include/bpmult_hip.h).

Torch CUDA tensors are used only for their device pointers.  Problem structs
are plain ctypes structures built once per (layer, op) and replayed every step
with a fresh dropout seed; the call is enqueued on torch's current stream and a
non-zero return code becomes a RuntimeError.  No arithmetic happens in Python,
and there is no CPU fallback.

Every entry point that takes an array of problems is launched by _grouped(): it
finds the problem struct in _lib.SIGNATURES, walks the array in chunks of the
library's group limit and calls entry(*pre, problems, count, *post, stream).

A launch-table step (engine.EncoderGroupPlan) is a tuple (fn, *args) with fn one
of STEP_FUNCTIONS; it is run as fn(*args, seed=seed) when fn is in SEEDED and as
fn(*args) otherwise.  Both sets are defined at the end of this module.
"""
from __future__ import annotations

import ctypes as C
import os
from typing import Optional, Sequence

import torch

from . import _lib
from ._lib import (BPM_BF16, BPM_BF16X3, BPM_F32, F_ACCUM, F_ATOMIC, F_KPAD, F_RELU, GEMM_NN, GEMM_NT, GEMM_TN, GEMM_MAX_GROUP, MAX_GROUP, OUT_CT,
                   OUT_F32, OUT_HEADS, AttnHeadMapProblem, AttnMapProblem, AttnProblem, CastProblem, EmbedProblem, GemmProblem, GmuProblem,
                   KvSourceProblem, LnProblem, PackProblem)


def pad32(n: int) -> int:
    return (n + 31) // 32 * 32


def ct_torch(dtype: int) -> torch.dtype:
    return torch.bfloat16 if dtype == BPM_BF16 else torch.float32


def _stream() -> int:
    return torch.cuda.current_stream().cuda_stream


class DeviceSeed(int):
    """A dropout seed the kernels read from device memory when they run (captured graphs): BPM_SEED_INDIRECT | address
    of a uint64.  Only values of this type may have bit 63 set; a plain int with that bit is rejected below instead of
    being dereferenced as a pointer on the device."""

    def __new__(cls, tensor: torch.Tensor):
        if tensor.dtype != torch.int64 or tensor.numel() < 1 or not (tensor.is_cuda or _DRY_RUN):
            raise ValueError("DeviceSeed: a CUDA int64 tensor holding the seed")
        return super().__new__(cls, _lib.SEED_INDIRECT | tensor.data_ptr())


def _seed(seed: int) -> int:
    if (seed & _lib.SEED_INDIRECT) and not isinstance(seed, DeviceSeed):
        raise ValueError("dropout seeds passed by value are 63-bit (bit 63 marks a device-resident seed: ops.DeviceSeed)")
    return int(seed)


# tests/test_plan_tables_cpu.py only: lets the launch TABLES (host logic: pointers, shapes, flags) be built from host
# tensors without a GPU.  Nothing can be launched from them -- every bpm_* entry point needs device pointers.
_DRY_RUN = False
# ... and the calls that are issued outside a plan's step tables (attn_maps) are recorded here instead of being launched
_DRY_LAUNCHES: list = []


def _p(t) -> Optional[int]:
    if t is None or isinstance(t, int):     # raw device address (e.g. an offset into a flat buffer)
        return t
    if not t.is_cuda and not _DRY_RUN:
        raise ValueError("expected a CUDA (HIP) tensor: the BPMulT hot path has no CPU fallback")
    return t.data_ptr()


def _f32(t, what):
    if t is not None and not isinstance(t, int) and t.dtype != torch.float32:
        raise ValueError(f"{what}: expected float32, got {t.dtype}")
    return _p(t)


def _counter(t, what):
    if t is not None and not isinstance(t, int) and (t.dtype != torch.int32 or t.numel() < 1):
        raise ValueError(f"{what}: an int32 device counter")
    return _p(t)


def _f32_table(t, what: str, d: int):
    """A [rows, d] table the kernels index by row: d floats per row, rows d floats apart (a view of whole rows is fine)."""
    if t.dtype != torch.float32 or t.dim() != 2 or t.shape[1] != d or t.stride() != (d, 1):
        raise ValueError(f"{what}: expected float32 [rows, {d}] with contiguous rows, got {t.dtype} {tuple(t.shape)}")
    return _p(t)


def _adam_scalars(what: str, ngroups: int, scale_dev, norm_dev, steps_dev, skipped_dev):
    """The device scalars of the Adam entries, checked -> their four addresses in the entries' order."""
    for t, nm in ((scale_dev, "scale_dev"), (norm_dev, "norm_dev")):
        if t is not None and (t.dtype != torch.float32 or t.numel() < 1):
            raise ValueError(f"{what}: {nm}: expected float32 (one device value), got {t.dtype}")
    if steps_dev is not None and (steps_dev.dtype != torch.int32 or steps_dev.numel() < ngroups or not steps_dev.is_contiguous()):
        raise ValueError(f"{what}: steps_dev: a contiguous tensor of one int32 device counter per group")
    return _p(scale_dev), _p(norm_dev), _p(steps_dev), _counter(skipped_dev, f"{what}: skipped_dev")


def array(cls, probs: Sequence):
    """ctypes array of problem structs (cache it; it is replayed every step)."""
    return (cls * len(probs))(*probs)


def _as_array(cls, probs):
    return probs if isinstance(probs, C.Array) else array(cls, probs)


def _at(arr, i: int):
    """Pointer to element i of a ctypes array."""
    return C.cast(C.byref(arr, i * C.sizeof(arr._type_)), C.POINTER(arr._type_))


_PROBLEM = {}       # entry point -> the struct of its problem array (the first POINTER(struct) of its signature)


def _grouped(name: str, probs, pre=(), post=(), limit: int = MAX_GROUP, beside=None, n: Optional[int] = None) -> None:
    """Launch the first n (default: all) problems through entry point `name`, `limit` at a time: one call
    entry(*pre, problems, [beside,] count, *post, stream) per chunk.  post: the scalars behind the count, or a function
    of the chunk's count that returns them; beside: a second ctypes array that advances with the problems, or a tuple of
    such arrays (in the entry's order)."""
    cls = _PROBLEM.get(name)
    if cls is None:
        cls = _PROBLEM[name] = next(t._type_ for t in _lib.SIGNATURES[name] if isinstance(t, type) and issubclass(t, C._Pointer))
    arr = _as_array(cls, probs)
    entry, s = getattr(_lib.lib(), name), _stream()
    n = len(arr) if n is None else n
    for i in range(0, n, limit):
        k = min(limit, n - i)
        also = () if beside is None else tuple(_at(b, i) for b in (beside if isinstance(beside, tuple) else (beside,)))
        _lib.check(entry(*pre, _at(arr, i), *also, k, *(post(k) if callable(post) else post), s), name)


# ----------------------------------------------------------------------------
# GEMM
# ----------------------------------------------------------------------------
def gemm_problem(A, B, Cc, M: int, N: int, K: int, lda: int, ldb: int, ldc: int, *, bias_n=None, bias_m=None,
                 resid=None, ldr: int = 0, gate=None, ldg: int = 0, gate_scale: float = 1.0, alpha: float = 1.0,
                 drop_p: float = 0.0, drop_site: int = 0, colsum=None, flags: int = 0, out_kind: int = OUT_F32,
                 splitk: int = 1, heads=None, colsum_a=None, batch=None) -> GemmProblem:
    """A, B, C: tensors or raw device addresses (int).  heads = (B, H, T, dh, dhp) for OUT_HEADS.
    batch = (n, stride_a, stride_b, stride_c): n products of this shape, operands / output of element i start i * stride
    elements further on (BPM_GEMM_BATCHED)."""
    p = GemmProblem()
    p.A, p.B, p.C = (x if isinstance(x, int) else _p(x) for x in (A, B, Cc))
    p.M, p.N, p.K = M, N, K
    p.lda, p.ldb, p.ldc = lda, ldb, ldc
    p.bias_n, p.bias_m = _f32(bias_n, "bias_n"), _f32(bias_m, "bias_m")
    p.resid, p.ldr = _f32(resid, "resid"), ldr
    p.gate, p.ldg, p.gate_scale = _p(gate), ldg, gate_scale
    p.alpha, p.drop_p, p.drop_site = alpha, drop_p, drop_site
    p.colsum = colsum if isinstance(colsum, int) else _f32(colsum, "colsum")
    p.flags, p.out_kind, p.splitk = flags, out_kind, splitk
    if heads is not None:
        p.heads_B, p.heads_H, p.heads_T, p.heads_dh, p.heads_dhp = heads
    p.colsum_a = colsum_a if isinstance(colsum_a, int) else _f32(colsum_a, "colsum_a")
    if batch is not None:
        p.batch, p.batch_stride_a, p.batch_stride_b, p.batch_stride_c = batch
        p.flags |= _lib.F_BATCHED
    return p


def gemm_grouped(dtype: int, variant: int, probs, seed: int = 0, n: Optional[int] = None, x3: "Optional[X3Cache]" = None) -> None:
    """x3 (or an array tagged `.x3 = <X3Cache>` where the launch tables are built): the parity-grade fast mode -- fp32
    operands, each product as three bf16 MFMA products of split operands (see _X3Plan), their split images held by that
    cache; launches the LDS-DMA kernel cannot take run as exact fp32 products.  None or False: the mode is off."""
    arr = _as_array(GemmProblem, probs)
    cache = x3 or getattr(arr, "x3", None) or None
    if cache is not None and not isinstance(cache, X3Cache):
        raise TypeError(f"x3: an ops.X3Cache (the owner of the split images) or None, got {type(cache).__name__}")
    if cache is not None and dtype == BPM_F32 and variant in _X3_VARIANTS:
        plan = getattr(arr, "_x3_plan", None)
        if plan is None or plan.n != n or plan.cache is not cache:
            plan = _X3Plan(arr, variant, n, cache)
            arr._x3_plan = plan              # tables are replayed every step; lists were turned into a fresh array above
        if plan.ok:
            plan.run(_lib.lib(), variant, _seed(seed), _stream())
            if plan.rest is None:
                return
            arr, n = plan.rest, None            # the problems the split path does not take: exact fp32 products
    _grouped("bpm_gemm_grouped", arr, (dtype, variant), (_seed(seed),), GEMM_MAX_GROUP, n=n)


# ---- bf16x3: fp32 products as three bf16 MFMA products of split operands -------------------------------------------
# x = hi + lo (hi = bf16(x), lo = bf16(x - hi)); x y ~ hi hi + hi lo + lo hi with f32 accumulation: ~2^-16 relative per
# product (the lo lo term and the rounding of lo), against 2^-9 for plain bf16 operands.  Every operand of an eligible
# launch is split by bpm_split_rows into a [rows, hi plane | lo plane] bf16 image (cached per operand view: the buffers
# of the hot path are static) right before the launch; weight shadows -- operands inside a static range of the cache that
# owns the weights -- are split again only after the shadows were refreshed.
# lab knob: BPMULT_X3_ONLY=nt,nn restricts the split path to those operand arrangements (bisecting a parity failure)
_X3_VARIANTS = {{"nt": GEMM_NT, "nn": GEMM_NN, "tn": GEMM_TN}[v] for v in os.environ.get("BPMULT_X3_ONLY", "nt,nn,tn").split(",") if v}


def _split(probs) -> None:
    _grouped("bpm_split_rows", probs)


class X3Cache:
    """The split images of one owner's operands (a trunk's or a stand-alone plan's activations, a ParamStore's weight
    shadows), held for as long as the owner lives.  `weights`: the cache that owns the static ranges -- operands that only
    change at a refresh -- with their images and SplitProblems (the store's; default: this one)."""

    def __init__(self, device, weights: "Optional[X3Cache]" = None):
        self.device = device
        self.weights = weights          # None: this cache itself (kept as None: a self-reference would leave the images to the gc)
        self.images = {}                # (ptr, rows, cols, ld) -> split image
        self.static = set()             # [lo, hi) address ranges of operands that only change at a refresh (weight shadows)
        self.static_splits = {}         # (ptr, rows, cols, ld) -> SplitProblem of every static operand seen so far
        self.epoch = 0                  # bumped once per forward pass (new_step)
        self.fresh = {}                 # operand key -> epoch of its last split (host program order)

    def add_static(self, lo: int, hi: int) -> None:
        self.static.add((lo, hi))

    def refresh_static(self) -> None:
        """Split every static operand again (ParamStore.refresh_shadows, after the weight shadows changed).  A host-side
        decision, outside any captured graph -- like the shadow refresh itself; the launch plans never split static operands
        except the first time they meet one."""
        if self.static_splits:
            _split(list(self.static_splits.values()))

    def new_step(self) -> None:
        self.epoch += 1


class _X3Plan:
    """Split problems + the BPM_BF16X3 problem table of one grouped GEMM launch (built once per launch table).
    Problems the split path does not take (fewer than 256 rows / columns / k, row bias, ...) stay behind in `rest` and run
    as exact fp32 products.  Operands listed in the table's `x3_presplit` attribute (set where the launch tables are
    built: forward activations a backward launch reads again, gradients an earlier launch of the same layer has split)
    are not split again when their image is from this step.  The plan holds its cache, and so the images it points into."""

    def __init__(self, arr, variant: int, n: Optional[int], cache: X3Cache):
        self.n, self.cache = n, cache
        cnt = len(arr) if n is None else n
        P = [arr[i] for i in range(cnt)]
        xk, yk = variant != GEMM_TN, variant == GEMM_NT
        take = [p for p in P if self._eligible(p)]
        if take and variant == GEMM_TN:               # one 256 x 256 tile per CU must roughly fill the chip (as in bf16 mode)
            if sum(((p.M + 255) // 256) * ((p.N + 255) // 256) for p in take) * 8 < 256 * 3:
                take = []
        self.ok = bool(take)
        self.rest = None
        self._keys = []
        if not self.ok:
            return
        if len(take) < cnt:
            ids = {C.addressof(p) for p in take}
            self.rest = array(GemmProblem, [p for p in P if C.addressof(p) not in ids])
        presplit = getattr(arr, "x3_presplit", ())
        weights = cache if cache.weights is None else cache.weights
        dyn, new_static, out = [], [], []
        seen = {}
        for p in take:
            q = GemmProblem()
            C.memmove(C.byref(q), C.byref(p), C.sizeof(GemmProblem))
            for side, rows, cols, ld in (("A", p.M if xk else p.K, p.K if xk else p.M, p.lda),
                                         ("B", p.N if yk else p.K, p.K if yk else p.N, p.ldb)):
                ptr = getattr(p, side)
                key = (ptr, rows, cols, ld)
                ldp = (cols + 127) // 128 * 128
                static = any(lo <= ptr < hi for lo, hi in weights.static)
                own = weights if static else cache            # a weight shadow's image belongs to the store's cache
                buf = own.images.get(key)
                if buf is None:
                    # torch.empty, NOT zeros: bpm_split_rows writes every column of both planes (pads included), and an
                    # initialising kernel on the allocating stream would race with the other stream's split of the same
                    # operand (main runs ahead of the side stream: its split + product would be wiped by the late fill)
                    buf = own.images[key] = torch.empty(rows, 2 * ldp, device=own.device, dtype=torch.bfloat16)
                if key not in seen:
                    seen[key] = True
                    sp = _lib.SplitProblem()
                    sp.src, sp.dst, sp.R, sp.C, sp.ld, sp.ldp = ptr, buf.data_ptr(), rows, cols, ld, ldp
                    if static:
                        if key not in own.static_splits:
                            own.static_splits[key] = sp
                            new_static.append(sp)
                    elif ptr in presplit and cache.fresh.get(key) == cache.epoch:
                        pass                          # an earlier launch of this step left the image (static launch order)
                    else:
                        dyn.append(sp)
                        self._keys.append(key)
                setattr(q, side, buf.data_ptr())
                setattr(q, "lda" if side == "A" else "ldb", 2 * ldp)
            q.flags |= F_KPAD
            out.append(q)
        self.gemm = array(GemmProblem, out)
        self.dyn = array(_lib.SplitProblem, dyn) if dyn else None
        if new_static:                                # first sight of a weight shadow: split it now (plans are built by eager
            _split(new_static)                        # launches, never inside a graph capture); later: refresh_static()

    @staticmethod
    def _eligible(p) -> bool:
        al = (p.bias_n or 0) | (p.resid or 0) | (p.C or 0) | (p.gate or 0)
        tm, tn = (p.M + 255) // 256, (p.N + 255) // 256
        return (p.M >= 256 and p.N >= 256 and p.K >= 256 and p.N % 4 == 0 and al % 16 == 0 and (p.ldr | p.ldc | p.ldg) % 4 == 0
                and not p.bias_m and p.splitk <= 1 and not (p.flags & (F_ATOMIC | _lib.F_A_OVERLAP | _lib.F_B_OVERLAP))
                and not (p.resid and (p.flags & F_ACCUM)) and p.M * p.N >= 0.8 * (tm * 256) * (tn * 256)
                and p.lda % 4 == 0 and p.ldb % 4 == 0 and (p.A or 0) % 16 == 0 and (p.B or 0) % 16 == 0)

    def run(self, L, variant: int, seed: int, s: int) -> None:
        if self.dyn is not None:
            _split(self.dyn)
            for key in self._keys:
                self.cache.fresh[key] = self.cache.epoch
        _lib.check(L.bpm_gemm_grouped(_lib.BPM_BF16X3, variant, self.gemm, len(self.gemm), seed, s), "bpm_gemm_grouped(bf16x3)")


# ----------------------------------------------------------------------------
# attention
# ----------------------------------------------------------------------------
def attn_problem(Q, K, V, O, ldo, lse, B, H, T, S, dh, dhp, mask_off, *, dO=None, delta=None, dQ=None, lddq=0,
                 dK=None, lddk=0, dV=None, lddv=0, dq_scale=1.0, drop_p=0.0, drop_site=0, q_pos0=0, q_stride=1,
                 dS=None, Pd=None, xs=(0, 0, 0)) -> AttnProblem:
    """dS / Pd (attn_bwd_dq only): CT tensors that receive the score gradient and the dropped probabilities, element
    (b, h, i, j) at b*xs[0] + h*xs[1] + i*xs[2] + j."""
    p = AttnProblem()
    p.q_pos0, p.q_stride = q_pos0, q_stride
    p.dS, p.Pd = _p(dS), _p(Pd)
    p.xs_b, p.xs_h, p.xs_q = xs
    p.Q, p.K, p.V, p.O, p.ldo, p.lse = _p(Q), _p(K), _p(V), _p(O), ldo, _f32(lse, "lse")
    p.dO, p.delta = _p(dO), _f32(delta, "delta")
    p.dQ, p.lddq, p.dK, p.lddk, p.dV, p.lddv = _p(dQ), lddq, _p(dK), lddk, _p(dV), lddv
    p.B, p.H, p.T, p.S, p.dh, p.dhp, p.mask_off = B, H, T, S, dh, dhp, mask_off
    p.dq_scale, p.drop_p, p.drop_site = dq_scale, drop_p, drop_site
    return p


def attn_fwd(dtype: int, probs, seed: int = 0) -> None:
    _grouped("bpm_attn_fwd", probs, (dtype,), (_seed(seed),))


def attn_bwd(dtype: int, probs, seed: int = 0) -> None:
    _grouped("bpm_attn_bwd", probs, (dtype,), (_seed(seed),))


def attn_bwd_dq(dtype: int, probs, seed: int = 0) -> None:
    _grouped("bpm_attn_bwd_dq", probs, (dtype,), (_seed(seed),))


def attn_bwd_dkv(dtype: int, probs, seed: int = 0) -> None:
    _grouped("bpm_attn_bwd_dkv", probs, (dtype,), (_seed(seed),))


def attn_kmasks(masks) -> "C.Array":
    """[(uint8 device tensor [B, ldm], ldm)] -> the host array of bpm_attn_kmask the *_kmask entries take beside the
    problems: key j of sample b is visible iff mask[b, j] != 0 (AND the problem's mask_off rule).  Every sample needs at
    least one visible key (not checked: the mask never travels to the host)."""
    arr = (_lib.AttnKMask * len(masks))()
    for a, (m, ldm) in zip(arr, masks):
        if not isinstance(m, int) and m.dtype != torch.uint8:
            raise ValueError(f"attention key mask: expected uint8, got {m.dtype}")
        a.mask, a.ldm = _p(m), ldm
    return arr


def _attn_kmask(name: str, dtype: int, probs, masks, seed: int) -> None:
    arr = _as_array(AttnProblem, probs)
    if len(masks) != len(arr):
        raise ValueError(f"{name}: one key mask per problem ({len(arr)} problems, {len(masks)} masks)")
    _grouped(name, arr, (dtype,), (_seed(seed),), beside=masks)


def attn_fwd_kmask(dtype: int, probs, masks, seed: int = 0) -> None:
    """bpm_attn_fwd with a per-key padding mask: `masks` from attn_kmasks(), one per problem."""
    _attn_kmask("bpm_attn_fwd_kmask", dtype, probs, masks, seed)


def attn_bwd_dq_kmask(dtype: int, probs, masks, seed: int = 0) -> None:
    _attn_kmask("bpm_attn_bwd_dq_kmask", dtype, probs, masks, seed)


def attn_bwd_dkv_kmask(dtype: int, probs, masks, seed: int = 0) -> None:
    _attn_kmask("bpm_attn_bwd_dkv_kmask", dtype, probs, masks, seed)


def attn_maps_kmask(dtype: int, probs, kmasks) -> None:
    """bpm_attn_maps after attn_fwd_kmask: `kmasks` from attn_kmasks(), one per problem; a key its byte hides is exactly 0."""
    arr = _as_array(AttnMapProblem, probs)
    if len(kmasks) != len(arr):
        raise ValueError(f"bpm_attn_maps_kmask: one key mask per problem ({len(arr)} problems, {len(kmasks)} masks)")
    if _DRY_RUN:
        _DRY_LAUNCHES.append((attn_maps_kmask, dtype, arr, kmasks))
        return
    _grouped("bpm_attn_maps_kmask", arr, (dtype,), beside=kmasks)


def attn_map_problem(Q, K, lse, W, ldw, B, H, T, S, dh, dhp, mask_off, *, q_pos0=0, q_stride=1) -> AttnMapProblem:
    """One head-averaged attention map (bpm_attn_maps): Q / K / lse as attn_problem's after its forward, W fp32 [B, T, ldw]
    receives (1/H) sum_h softmax probabilities (before dropout; exactly 0 where the mask hides the key)."""
    p = AttnMapProblem()
    p.Q, p.K, p.lse, p.W, p.ldw = _p(Q), _p(K), _f32(lse, "lse"), _f32(W, "W"), ldw
    p.B, p.H, p.T, p.S, p.dh, p.dhp, p.mask_off = B, H, T, S, dh, dhp, mask_off
    p.q_pos0, p.q_stride = q_pos0, q_stride
    return p


def attn_maps(dtype: int, probs) -> None:
    arr = _as_array(AttnMapProblem, probs)
    if _DRY_RUN:
        _DRY_LAUNCHES.append((attn_maps, dtype, arr))
        return
    _grouped("bpm_attn_maps", arr, (dtype,))


def attn_amasks(masks) -> "C.Array":
    """[(mask, ldm, maskT, ldt)] or [(mask, ldm, maskT, ldt, head_stride, head_strideT)] -> the host array of
    bpm_attn_hmask (bpm_attn_amask plus the two head strides; the attn_*_amask wrappers below launch through the *_hmask
    entries, which are the *_amask entries at stride 0) that they take beside the problems.  A third form, the 8-tuple
    (mask, ldm, maskT, ldt, head_stride, head_strideT, batch_stride, batch_strideT), builds bpm_attn_bmask instead: sample b
    reads the image(s) at mask + b * batch_stride (maskT + b * batch_strideT), and every wrapper that takes the array
    launches through the *_bmask / *_kbmask entry of its family.  mask: float32 device tensor [T, ldm] added to the scores
    of every head (-inf hides the pair; AND the problem's mask_off rule), ldm >= S and a multiple of 4, 16-byte aligned;
    maskT: its transpose [S, ldt] under the same rules, which the dK / dV and maps entries read (None, 0 for forward / dQ
    only).  The head strides (elements; the 4-tuple form: 0) turn them into H images [H, T, ldm] / [H, S, ldt], head h of
    every sample reading its own.  Every query row needs a visible key (not checked)."""
    per_sample = any(len(t) == 8 for t in masks)
    arr = ((_lib.AttnBMask if per_sample else _lib.AttnHMask) * len(masks))()
    for a, t in zip(arr, masks):
        m, ldm, mt, ldt = t[:4]
        hs, hst = t[4:6] if len(t) >= 6 else (0, 0)
        a.mask, a.ldm, a.maskT, a.ldt = _f32(m, "additive attention mask"), ldm, _f32(mt, "additive attention mask (transpose)"), ldt
        a.head_stride, a.head_strideT = hs, hst
        if per_sample:
            a.batch_stride, a.batch_strideT = t[6:] if len(t) == 8 else (0, 0)
    return arr


def _per_sample(masks) -> bool:
    """The array came from the 8-tuple form of attn_amasks() (bpm_attn_bmask) or the 4-tuple form of attn_dbias()."""
    return getattr(masks, "_type_", None) in (_lib.AttnBMask, _lib.AttnDBiasB)


def _mask_entry(name: str, masks) -> str:
    """The entry that takes these additive masks: the *_hmask / *_kamask one, or its per-sample sibling *_bmask / *_kbmask."""
    if _per_sample(masks):
        return name.replace("_kamask", "_kbmask").replace("_hmask", "_bmask")
    return name


def _attn_amask(name: str, dtype: int, probs, masks, seed: int) -> None:
    arr = _as_array(AttnProblem, probs)
    if len(masks) != len(arr):
        raise ValueError(f"{name}: one additive mask per problem ({len(arr)} problems, {len(masks)} masks)")
    _grouped(_mask_entry(name.replace("_amask", "_hmask"), masks), arr, (dtype,), (_seed(seed),), beside=masks)


def attn_fwd_amask(dtype: int, probs, masks, seed: int = 0) -> None:
    """bpm_attn_fwd with an additive [T, S] mask: `masks` from attn_amasks(), one per problem."""
    _attn_amask("bpm_attn_fwd_amask", dtype, probs, masks, seed)


def attn_bwd_dq_amask(dtype: int, probs, masks, seed: int = 0) -> None:
    _attn_amask("bpm_attn_bwd_dq_amask", dtype, probs, masks, seed)


def attn_bwd_dkv_amask(dtype: int, probs, masks, seed: int = 0) -> None:
    _attn_amask("bpm_attn_bwd_dkv_amask", dtype, probs, masks, seed)


def attn_maps_amask(dtype: int, probs, masks) -> None:
    arr = _as_array(AttnMapProblem, probs)
    if len(masks) != len(arr):
        raise ValueError(f"bpm_attn_maps_amask: one additive mask per problem ({len(arr)} problems, {len(masks)} masks)")
    _grouped(_mask_entry("bpm_attn_maps_hmask", masks), arr, (dtype,), beside=masks)


def _attn_kamask(name: str, dtype: int, probs, kmasks, masks, seed: int) -> None:
    arr = _as_array(AttnProblem, probs)
    if len(kmasks) != len(arr) or len(masks) != len(arr):
        raise ValueError(f"{name}: one key mask and one additive mask per problem ({len(arr)} problems, {len(kmasks)} key masks, "
                         f"{len(masks)} additive masks)")
    _grouped(_mask_entry(name, masks), arr, (dtype,), (_seed(seed),), beside=(kmasks, masks))


def attn_fwd_kamask(dtype: int, probs, kmasks, masks, seed: int = 0) -> None:
    """bpm_attn_fwd with a per-key padding mask AND an additive mask: `kmasks` from attn_kmasks(), `masks` from
    attn_amasks(), one of each per problem.  A pair is visible iff the mask_off rule, the key's byte and the additive entry
    (> -inf) all say so; every query row of every sample needs a visible key (not checked)."""
    _attn_kamask("bpm_attn_fwd_kamask", dtype, probs, kmasks, masks, seed)


def attn_bwd_dq_kamask(dtype: int, probs, kmasks, masks, seed: int = 0) -> None:
    _attn_kamask("bpm_attn_bwd_dq_kamask", dtype, probs, kmasks, masks, seed)


def attn_bwd_dkv_kamask(dtype: int, probs, kmasks, masks, seed: int = 0) -> None:
    _attn_kamask("bpm_attn_bwd_dkv_kamask", dtype, probs, kmasks, masks, seed)


def attn_maps_kamask(dtype: int, probs, kmasks, masks) -> None:
    arr = _as_array(AttnMapProblem, probs)
    if len(kmasks) != len(arr) or len(masks) != len(arr):
        raise ValueError(f"bpm_attn_maps_kamask: one key mask and one additive mask per problem ({len(arr)} problems, "
                         f"{len(kmasks)} key masks, {len(masks)} additive masks)")
    if _DRY_RUN:
        _DRY_LAUNCHES.append((attn_maps_kamask, dtype, arr, kmasks, masks))
        return
    _grouped(_mask_entry("bpm_attn_maps_kamask", masks), arr, (dtype,), beside=(kmasks, masks))


def attn_head_map_problem(Q, K, lse, W, ldw, B, H, T, S, dh, dhp, mask_off, *, q_pos0=0, q_stride=1, head_stride=None,
                          batch_stride=None) -> AttnHeadMapProblem:
    """One per-head attention map (bpm_attn_head_maps): attn_map_problem with W fp32 [B, H, T, ldw], which receives the
    softmax probabilities of every head (before dropout; exactly 0 where a mask hides the pair) -- H times the bytes of
    the averaged map.  head_stride / batch_stride (elements; default: the dense T * ldw and H * head_stride) place the map
    of (sample b, head h) at W + b * batch_stride + h * head_stride."""
    p = AttnHeadMapProblem()
    p.Q, p.K, p.lse, p.W, p.ldw = _p(Q), _p(K), _f32(lse, "lse"), _f32(W, "W"), ldw
    p.B, p.H, p.T, p.S, p.dh, p.dhp, p.mask_off = B, H, T, S, dh, dhp, mask_off
    p.q_pos0, p.q_stride = q_pos0, q_stride
    p.head_stride = T * ldw if head_stride is None else head_stride
    p.batch_stride = H * p.head_stride if batch_stride is None else batch_stride
    return p


def _attn_head_maps(fn, name: str, dtype: int, probs, *beside) -> None:
    """The five per-head map launches: as their attn_maps* siblings (outside the step tables: recorded in dry mode)."""
    arr = _as_array(AttnHeadMapProblem, probs)
    if any(len(b) != len(arr) for b in beside):
        raise ValueError(f"{name}: one mask of each kind per problem ({len(arr)} problems, {' / '.join(str(len(b)) for b in beside)} masks)")
    if _DRY_RUN:
        _DRY_LAUNCHES.append((fn, dtype, arr, *beside))
        return
    if beside:
        name = _mask_entry(name, beside[-1])
    _grouped(name, arr, (dtype,), beside=beside if len(beside) > 1 else (beside[0] if beside else None))


def attn_head_maps(dtype: int, probs) -> None:
    _attn_head_maps(attn_head_maps, "bpm_attn_head_maps", dtype, probs)


def attn_head_maps_kmask(dtype: int, probs, kmasks) -> None:
    """bpm_attn_head_maps after attn_fwd_kmask: `kmasks` from attn_kmasks(), one per problem."""
    _attn_head_maps(attn_head_maps_kmask, "bpm_attn_head_maps_kmask", dtype, probs, kmasks)


def attn_head_maps_hmask(dtype: int, probs, masks) -> None:
    """bpm_attn_head_maps after attn_fwd_amask / _hmask: `masks` from attn_amasks() (with their transposes), one per problem."""
    _attn_head_maps(attn_head_maps_hmask, "bpm_attn_head_maps_hmask", dtype, probs, masks)


def attn_head_maps_amask(dtype: int, probs, masks) -> None:
    """attn_head_maps_hmask: attn_amasks() builds bpm_attn_hmask, and the *_amask entry is the *_hmask entry at stride 0."""
    _attn_head_maps(attn_head_maps_amask, "bpm_attn_head_maps_hmask", dtype, probs, masks)


def attn_head_maps_kamask(dtype: int, probs, kmasks, masks) -> None:
    _attn_head_maps(attn_head_maps_kamask, "bpm_attn_head_maps_kamask", dtype, probs, kmasks, masks)


def attn_dbias(outs) -> "C.Array":
    """[(dB, lddb, head_stride)] -> the host array of bpm_attn_dbias that bpm_attn_bwd_dbias takes beside the problems and
    their masks.  dB: float32 device tensor [T, lddb] (head_stride 0: the gradient summed over samples and heads) or
    [H, T, lddb] with head_stride elements between the images (summed over samples), lddb >= S and a multiple of 4,
    16-byte aligned.  Columns >= S are left alone.  The 4-tuple form (dB, lddb, head_stride, batch_stride) builds
    bpm_attn_dbias_b: a non-zero batch_stride keeps the samples apart -- [B, H, T, lddb] (dB[b, h] = dS[b, h]) or, with
    head_stride 0, [B, 1, T, lddb] (summed over the heads of sample b) -- through bpm_attn_bwd_dbias_bmask."""
    per_sample = any(len(t) == 4 for t in outs)
    arr = ((_lib.AttnDBiasB if per_sample else _lib.AttnDBias) * len(outs))()
    for a, t in zip(arr, outs):
        a.dB, a.lddb, a.head_stride = _f32(t[0], "attention bias gradient"), t[1], t[2]
        if per_sample:
            a.batch_stride = t[3] if len(t) == 4 else 0
    return arr


def _as_bmasks(masks) -> "C.Array":
    """bpm_attn_hmask array -> the same masks as bpm_attn_bmask at batch stride 0 (for the per-sample bias gradient)."""
    if _per_sample(masks):
        return masks
    arr = (_lib.AttnBMask * len(masks))()
    for a, m in zip(arr, masks):
        a.mask, a.ldm, a.maskT, a.ldt, a.head_stride, a.head_strideT = m.mask, m.ldm, m.maskT, m.ldt, m.head_stride, m.head_strideT
    return arr


def attn_dbias_ws_bytes(probs, outs) -> int:
    """Bytes of workspace bpm_attn_bwd_dbias needs for these problems (0: the head sums are not split)."""
    arr = _as_array(AttnProblem, probs)
    if len(outs) != len(arr):
        raise ValueError(f"bpm_attn_bwd_dbias_ws_bytes: one output per problem ({len(arr)} problems, {len(outs)} outputs)")
    if len(arr) > MAX_GROUP:
        raise ValueError(f"bpm_attn_bwd_dbias: at most {MAX_GROUP} problems per launch")
    if _per_sample(outs):
        return int(_lib.lib().bpm_attn_bwd_dbias_bmask_ws_bytes(arr, outs, len(arr)))
    return int(_lib.lib().bpm_attn_bwd_dbias_ws_bytes(arr, outs, len(arr)))


def attn_bwd_dbias(dtype: int, probs, masks, outs, seed: int = 0, ws=None, kmasks=None) -> None:
    """The gradient of the additive masks (`masks` from attn_amasks(), as the forward pass took them) into `outs` (from
    attn_dbias()), after attn_bwd_dq[_amask] has left delta.  ws: a device tensor of at least attn_dbias_ws_bytes() bytes
    (None when that is 0); one launch, so at most MAX_GROUP problems.  kmasks: the key masks (attn_kmasks()) of a forward
    pass through attn_fwd_kamask -- sample b adds nothing at the keys its byte hides (bpm_attn_bwd_dbias_kmask)."""
    arr = _as_array(AttnProblem, probs)
    if len(masks) != len(arr) or len(outs) != len(arr):
        raise ValueError(f"bpm_attn_bwd_dbias: one mask and one output per problem ({len(arr)} problems, {len(masks)} masks, {len(outs)} outputs)")
    if kmasks is not None and len(kmasks) != len(arr):
        raise ValueError(f"bpm_attn_bwd_dbias_kmask: one key mask per problem ({len(arr)} problems, {len(kmasks)} masks)")
    if len(arr) > MAX_GROUP:
        raise ValueError(f"bpm_attn_bwd_dbias: at most {MAX_GROUP} problems per launch")
    nbytes = 0 if ws is None else ws.numel() * ws.element_size()
    if _per_sample(masks) or _per_sample(outs):
        # per-sample masks or a per-sample result: the one entry that takes both (a shared form of either goes in at stride 0)
        if not _per_sample(outs):
            b = (_lib.AttnDBiasB * len(outs))()
            for d, o in zip(b, outs):
                d.dB, d.lddb, d.head_stride = o.dB, o.lddb, o.head_stride
            outs = b
        _lib.check(_lib.lib().bpm_attn_bwd_dbias_bmask(dtype, arr, _as_bmasks(masks), kmasks, outs, len(arr), _seed(seed), _p(ws), nbytes,
                                                       _stream()), "bpm_attn_bwd_dbias_bmask")
    elif kmasks is None:
        _lib.check(_lib.lib().bpm_attn_bwd_dbias(dtype, arr, masks, outs, len(arr), _seed(seed), _p(ws), nbytes, _stream()), "bpm_attn_bwd_dbias")
    else:
        _lib.check(_lib.lib().bpm_attn_bwd_dbias_kmask(dtype, arr, masks, kmasks, outs, len(arr), _seed(seed), _p(ws), nbytes, _stream()),
                   "bpm_attn_bwd_dbias_kmask")


# ----------------------------------------------------------------------------
# row kernels
# ----------------------------------------------------------------------------
def pack_problem(B, T, Cn, ld, *, src=None, dst=None, g=None, ldg=0, dsrc=None, drop_p=0.0, drop_site=0) -> PackProblem:
    p = PackProblem()
    p.src, p.dst, p.g, p.ldg, p.dsrc = _f32(src, "pack.src"), _p(dst), _f32(g, "pack.g"), ldg, _f32(dsrc, "pack.dsrc")
    p.B, p.T, p.C, p.ld, p.drop_p, p.drop_site = B, T, Cn, ld, drop_p, drop_site
    return p


def pack_rows_fwd(dtype, probs, seed=0) -> None:
    _grouped("bpm_pack_rows_fwd", probs, (dtype,), (_seed(seed),))


def pack_rows_bwd(probs, seed=0) -> None:
    _grouped("bpm_pack_rows_bwd", probs, (), (_seed(seed),))


def pack_weights(dtype, table_dev: torch.Tensor, ndesc: int, total_blocks: int) -> None:
    _lib.check(_lib.lib().bpm_pack_weights(dtype, table_dev.data_ptr(), ndesc, total_blocks, _stream()), "bpm_pack_weights")


def device_table(descs) -> torch.Tensor:
    """ctypes descriptor structs -> one device-resident byte tensor (the table-driven launches read it on the GPU)."""
    arr = (type(descs[0]) * len(descs))(*descs)
    t = torch.frombuffer(bytearray(bytes(memoryview(arr))), dtype=torch.uint8)
    return t if _DRY_RUN else t.to("cuda")


# Blocks a segment takes in a table-driven launch: the library's answer, or under _DRY_RUN (tables built without a GPU)
# its restatement: csrc/adam.hip's ADAM_CHUNK and SSQ_CHUNK (the segment's offset in its 16-byte line counts).
# bpm_zero_segment_blocks has none: a dry run asks whatever stands in for the library, and the block counts that
# tools/step_trace.py records are its stand-in's, not the library's
_DRY_BLOCKS = {"bpm_adam_blocks": lambda n4: (n4 + 1023) // 1024,
               "bpm_grad_sumsq_blocks": lambda ptr, n: ((ptr >> 2 & 3) + n + 4095) // 4096}


def _blocks(name: str, *args) -> int:
    if _DRY_RUN and name in _DRY_BLOCKS:
        return _DRY_BLOCKS[name](*args)
    return int(getattr(_lib.lib(), name)(*args))


def adam_blocks(n4: int) -> int:
    return _blocks("bpm_adam_blocks", n4)


def adam_groups(groups) -> "C.Array":
    """[{lr, betas, eps, weight_decay, decoupled_weight_decay, step}] -> the host array bpm_adam_step_groups takes."""
    if not 1 <= len(groups) <= _lib.ADAM_MAX_GROUPS:
        raise ValueError(f"adam_groups: 1 .. {_lib.ADAM_MAX_GROUPS} groups, got {len(groups)}")
    arr = (_lib.AdamGroup * len(groups))()
    for a, g in zip(arr, groups):
        a.lr, (a.beta1, a.beta2), a.eps, a.weight_decay = g["lr"], g["betas"], g["eps"], g["weight_decay"]
        a.decoupled, a.step = int(bool(g.get("decoupled_weight_decay", False))), int(g.get("step", 0))
    return arr


def adam_step_groups(dtype, table_dev, nseg, nblk, master, grad, exp_avg, exp_avg_sq, groups, grad_scale, zero_grad, scale_dev=None,
                     norm_dev=None, steps_dev=None, skipped_dev=None) -> None:
    """bpm_adam_step_groups: `groups` from adam_groups(); scale_dev / norm_dev: float32 device values (grad_sumsq's
    coefficient and norm); steps_dev: int32[len(groups)] device counters of applied steps; skipped_dev: one int32."""
    for t in (master, grad, exp_avg, exp_avg_sq):
        if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != master.numel():
            raise ValueError("adam_step_groups: flat contiguous float32 buffers of one size")
    scalars = _adam_scalars("adam_step_groups", len(groups), scale_dev, norm_dev, steps_dev, skipped_dev)
    _lib.check(_lib.lib().bpm_adam_step_groups(dtype, table_dev.data_ptr(), nseg, nblk, _p(master), _p(grad), _p(exp_avg), _p(exp_avg_sq),
                                               groups, len(groups), grad_scale, *scalars, int(bool(zero_grad)), _stream()),
               "bpm_adam_step_groups")


def adam_sets(buffers):
    """[(master, grad, exp_avg, exp_avg_sq)] flat float32 buffers, one tuple per set -> (device array, host array, the
    tensors) for adam_step_sets: the kernel reads the device array, the entry's checks the host one."""
    if not 1 <= len(buffers) <= _lib.ADAM_MAX_SETS:
        raise ValueError(f"adam_sets: 1 .. {_lib.ADAM_MAX_SETS} buffer sets, got {len(buffers)}")
    arr = (_lib.AdamSet * len(buffers))()
    for a, bufs in zip(arr, buffers):
        for t in bufs:
            if t.dtype != torch.float32 or not t.is_contiguous() or t.numel() != bufs[0].numel():
                raise ValueError("adam_sets: every set is four flat contiguous float32 buffers of one size")
        a.param, a.grad, a.exp_avg, a.exp_avg_sq = (_p(t) for t in bufs)
        a.n = bufs[0].numel()
    return device_table(list(arr)), arr, [tuple(b) for b in buffers]


def adam_sets_table(segments):
    """[AdamSeg] with group words from _lib.adam_set_group(), blk0 filled in here -> (device table, host array, segments,
    blocks) for adam_step_sets."""
    arr = (_lib.AdamSeg * len(segments))(*segments)
    blk = 0
    for sg in arr:
        sg.blk0 = blk
        blk += adam_blocks(sg.n4)
    return device_table(list(arr)), arr, len(arr), blk


def adam_step_sets(dtype, table, sets, groups, grad_scale, zero_grad, scale_dev=None, norm_dev=None, steps_dev=None,
                   skipped_dev=None) -> None:
    """bpm_adam_step_sets: adam_step_groups over several buffer sets in one launch.  table = adam_sets_table(...), sets =
    adam_sets(...), everything else as adam_step_groups."""
    table_dev, table_host, nseg, nblk = table
    sets_dev, sets_host, _ = sets
    scalars = _adam_scalars("adam_step_sets", len(groups), scale_dev, norm_dev, steps_dev, skipped_dev)
    _lib.check(_lib.lib().bpm_adam_step_sets(dtype, table_dev.data_ptr(), table_host, nseg, nblk, sets_dev.data_ptr(), sets_host,
                                             len(sets_host), groups, len(groups), grad_scale, *scalars, int(bool(zero_grad)), _stream()),
               "bpm_adam_step_sets")


def grad_sumsq_blocks(ptr: int, n: int) -> int:
    return _blocks("bpm_grad_sumsq_blocks", ptr, n)


def sumsq_table(segments):
    """[(device address, element count)] -> (device table, nseg, total blocks) for grad_sumsq."""
    descs, blk = [], 0
    for ptr, n in segments:
        if n < 1 or ptr % 4:
            raise ValueError("sumsq_table: segments of at least one float at 4-byte aligned addresses")
        sg = _lib.SumsqSeg()
        sg.p, sg.n, sg.blk0 = ptr, n, blk
        blk += grad_sumsq_blocks(ptr, n)
        descs.append(sg)
    return device_table(descs), len(descs), blk


def grad_sumsq_ws_bytes(total_blocks: int) -> int:
    return int(_lib.lib().bpm_grad_sumsq_ws_bytes(total_blocks))


def grad_sumsq(table_dev: torch.Tensor, nseg: int, total_blocks: int, ws: torch.Tensor, out: torch.Tensor, grad_scale: float = 1.0,
               max_norm: float = 0.0, extra_sumsq: Optional[torch.Tensor] = None) -> None:
    """out[0] = grad_scale * sqrt(sum of squares over the table + extra_sumsq), out[1] = torch's clip coefficient for
    max_norm (1 when max_norm <= 0 or inf); nothing leaves the device."""
    if out.dtype != torch.float32 or out.numel() < 2 or not out.is_contiguous():
        raise ValueError("grad_sumsq: out is a contiguous float32 tensor of two elements")
    if extra_sumsq is not None and (extra_sumsq.dtype != torch.float32 or extra_sumsq.numel() != 1):
        raise ValueError("grad_sumsq: extra_sumsq is one float32 device value")
    _lib.check(_lib.lib().bpm_grad_sumsq(table_dev.data_ptr(), nseg, total_blocks, grad_scale, max_norm, _p(extra_sumsq), _p(ws),
                                         ws.numel() * ws.element_size(), _p(out), _stream()), "bpm_grad_sumsq")


def fold_bias(table_dev: torch.Tensor, ndesc: int, total_blocks: int) -> None:
    _lib.check(_lib.lib().bpm_fold_bias(table_dev.data_ptr(), ndesc, total_blocks, _stream()), "bpm_fold_bias")


def unfold_grads(table_dev: torch.Tensor, ndesc: int, total_blocks: int, store_dw: bool = False) -> None:
    _lib.check(_lib.lib().bpm_unfold_grads(table_dev.data_ptr(), ndesc, total_blocks, int(store_dw), _stream()), "bpm_unfold_grads")


_UNFOLD_WS = {}
_WS_RETIRED: list = []      # replaced workspaces of every row entry: a captured graph may still hold their addresses


def _unfold_workspace(need: int, device) -> torch.Tensor:
    """Per-(device, stream) partial-row workspace of bpm_unfold_grads_ws, as _ln_workspace: launches on one stream are
    serialised and share it.  (The entry clears its ticket words itself.)  A workspace that a larger one replaces is
    kept: a captured graph may still hold its address (a few MB each, one per growth step)."""
    key = (str(device), _stream())
    t = _UNFOLD_WS.get(key)
    if t is None or t.numel() * 4 < need:
        if t is not None:
            _WS_RETIRED.append(t)
        t = torch.zeros((need + 3) // 4, device=device, dtype=torch.float32)
        _UNFOLD_WS[key] = t
    return t


def unfold_grads_ws(table_dev: torch.Tensor, ndesc: int, total_blocks: int, max_cols: int, store_dw: bool = False) -> None:
    """unfold_grads without float atomics (deterministic mode): dgamma / dbeta from per-block partial rows, added in block
    order by one owner.  max_cols: the widest descriptor's cols."""
    L = _lib.lib()
    ws = _unfold_workspace(L.bpm_unfold_grads_ws_bytes(ndesc, total_blocks, max_cols), table_dev.device)
    _lib.check(L.bpm_unfold_grads_ws(table_dev.data_ptr(), ndesc, total_blocks, int(store_dw), max_cols, ws.data_ptr(),
                                     ws.numel() * 4, _stream()), "bpm_unfold_grads_ws")


def zero_table(segments):
    """[(device address, element count)] -> (device table, ndesc, total blocks) for zero_segments."""
    descs, blk = [], 0
    for ptr, n in segments:
        z = _lib.ZeroDesc()
        z.p, z.n, z.blk0 = ptr, n, blk
        blk += _blocks("bpm_zero_segment_blocks", n)
        descs.append(z)
    return device_table(descs), len(descs), blk


def zero_segments(table_dev: torch.Tensor, ndesc: int, total_blocks: int) -> None:
    _lib.check(_lib.lib().bpm_zero_segments(table_dev.data_ptr(), ndesc, total_blocks, _stream()), "bpm_zero_segments")


def embed_problem(x, out, T, B, *, accumulate=False, drop_p=0.0, drop_site=0, pos0=0, pos_stride=1) -> EmbedProblem:
    p = EmbedProblem()
    p.x, p.out, p.T, p.B = _f32(x, "embed.x"), _f32(out, "embed.out"), T, B
    p.accumulate, p.drop_p, p.drop_site = int(accumulate), drop_p, drop_site
    p.pos0, p.pos_stride = pos0, pos_stride
    return p


def embed_pos_fwd(probs, table, d, scale, seed=0) -> None:
    _grouped("bpm_embed_pos_fwd", probs, (), (_f32_table(table, "embed_pos_fwd: table", d), table.shape[0], d, scale, _seed(seed)))


def embed_pos_bwd(probs, d, scale, seed=0) -> None:
    _grouped("bpm_embed_pos_bwd", probs, (), (d, scale, _seed(seed)))


def kv_source_ok(d: int, T: int, B: int) -> bool:
    """Shape domain of bpm_kv_source_fwd / _bwd (the pointers' 16-byte alignment is checked by the library)."""
    return d % 4 == 0 and 4 <= d <= 1024 and T * B * d < 1 << 32


def kv_source_problem(xk, xv, T, B, *, khat=None, vhat=None, ld=0, stats_k=(None, None), stats_v=(None, None), gk=None, gv=None,
                      dxk=None, dxv=None, drop_p=0.0, drop_site_k=0, drop_site_v=0, pos0=0, pos_stride=1) -> KvSourceProblem:
    """One key / value source of bpm_kv_source_fwd / _bwd (both directions read the same struct).  xk / xv may be None while
    a table is built and set before the launch (set_kv_source); dxv None (or dxk): the backward writes dxk = d(xk) + d(xv)."""
    p = KvSourceProblem()
    p.xk, p.xv, p.T, p.B, p.pos0, p.pos_stride = _f32(xk, "kv_source.xk"), _f32(xv, "kv_source.xv"), T, B, pos0, pos_stride
    p.drop_p_k, p.drop_site_k, p.drop_p_v, p.drop_site_v = drop_p, drop_site_k, drop_p, drop_site_v
    p.khat, p.vhat, p.ld = _p(khat), _p(vhat), ld
    p.mean_k, p.rstd_k = _f32(stats_k[0], "kv_source.mean_k"), _f32(stats_k[1], "kv_source.rstd_k")
    p.mean_v, p.rstd_v = _f32(stats_v[0], "kv_source.mean_v"), _f32(stats_v[1], "kv_source.rstd_v")
    p.gk, p.gv = _f32(gk, "kv_source.gk"), _f32(gv, "kv_source.gv")
    p.dxk, p.dxv = _f32(dxk, "kv_source.dxk"), _f32(dxv, "kv_source.dxv")
    return p


def set_kv_source(p: KvSourceProblem, xk, xv) -> None:
    p.xk, p.xv = _f32(xk, "kv_source.xk"), _f32(xv, "kv_source.xv")


def kv_source_fwd(dtype, probs, table, d, scale, seed=0, eps=1e-5) -> None:
    _grouped("bpm_kv_source_fwd", probs, (dtype,), (_f32_table(table, "kv_source: table", d), table.shape[0], d, scale, eps, _seed(seed)))


def kv_source_bwd(probs, table, d, scale, seed=0) -> None:
    _grouped("bpm_kv_source_bwd", probs, (), (_f32_table(table, "kv_source: table", d), table.shape[0], d, scale, _seed(seed)))


def ln_problem(x, gamma, beta, mean, rstd, R, *, out=None, ldo=0, out_f32=False, dy=None, ldy=0, add=None, dx=None,
               dgamma=None, dbeta=None, cast=None, ldc=0, cast_colsum=None, drop_p=0.0, drop_site=0) -> LnProblem:
    p = LnProblem()
    p.x, p.gamma, p.beta = _f32(x, "ln.x"), _f32(gamma, "ln.gamma"), _f32(beta, "ln.beta")
    p.out, p.ldo, p.out_f32 = _p(out), ldo, int(out_f32)
    p.mean, p.rstd, p.R = _f32(mean, "ln.mean"), _f32(rstd, "ln.rstd"), R
    p.dy, p.ldy, p.add, p.dx = _f32(dy, "ln.dy"), ldy, _f32(add, "ln.add"), _f32(dx, "ln.dx")
    p.dgamma, p.dbeta = _f32(dgamma, "ln.dgamma"), _f32(dbeta, "ln.dbeta")
    p.cast, p.ldc = _p(cast), ldc
    p.cast_colsum = cast_colsum if isinstance(cast_colsum, int) else _f32(cast_colsum, "ln.cast_colsum")
    p.drop_p, p.drop_site = drop_p, drop_site
    return p


def ln_fwd(dtype, probs, d, eps=1e-5) -> None:
    _grouped("bpm_ln_fwd", probs, (dtype,), (d, eps))


def check_ln_rows(probs, d: int) -> None:
    """Host-side contract of bpm_ln_bwd_ws for one launch group, checked where the launch TABLES are built (not per
    step): the dgamma / dbeta / cast_colsum rows ([d] floats each) of its problems are pairwise disjoint.  The last block
    of a problem adds its partial sums with a plain read-modify-write; the library detects EQUAL row pointers and falls
    back to atomics, but rows that overlap partially would be summed wrongly without any error."""
    rows = []
    for i, p in enumerate(probs):
        for nm in ("dgamma", "dbeta", "cast_colsum"):
            a = getattr(p, nm)
            if a and (nm != "cast_colsum" or p.cast):
                rows.append((int(a), i, nm))
    rows.sort()
    for (a, i, n1), (b, j, n2) in zip(rows, rows[1:]):
        if b < a + 4 * d:
            raise ValueError(f"ln_bwd group: {n1} of problem {i} and {n2} of problem {j} share gradient words "
                             f"(0x{a:x}, 0x{b:x}; rows are {4 * d} bytes): one launch must own each row exactly once")


_LN_WS = {}


def _ln_workspace(n: int, d: int, device, entry: str = "bpm_ln_bwd_ws_bytes") -> torch.Tensor:
    """Per-(device, stream) partial-sum workspace of bpm_ln_bwd_ws: launches on one stream are serialised, so they
    can share it; the side stream gets its own.  entry: the size query (bpm_ln_bwd_det's serves either of its routes, at
    twice the size: deterministic launches keep a workspace of their own, so they do not grow the default one).  A
    workspace that a larger one replaces is kept: a captured graph may still hold its address."""
    key = (str(device), _stream()) + (() if entry == "bpm_ln_bwd_ws_bytes" else (entry,))
    need = getattr(_lib.lib(), entry)(n, d)
    t = _LN_WS.get(key)
    if t is None or t.numel() * 4 < need:
        if t is not None:
            _WS_RETIRED.append(t)
        t = torch.zeros((need + 3) // 4, device=device, dtype=torch.float32)      # ticket words must start at zero
        _LN_WS[key] = t
    return t


def ln_det(probs):
    """The problems of a LayerNorm-backward STEP of a deterministic plan, marked where the launch table is built (a step
    is (fn, *args) run with the seed as its only keyword, and the seeded step functions are a fixed set: the mode
    travels on the array, as the bf16x3 flags of a GEMM step's array do).  EncoderGroupPlan.__init__ refuses a
    deterministic plan with an unmarked LayerNorm-backward step."""
    probs = _as_array(LnProblem, probs)
    probs.det = True
    return probs


def ln_bwd(probs, d, dtype=None, seed=0, deterministic: bool = False) -> None:
    """dtype / seed only matter for problems with a fused `cast` output.  Parameter / bias gradients go through a
    partial-sum workspace where the library can (no float atomics); deterministic (or an array marked by ln_det):
    through bpm_ln_bwd_det, which computes them without atomics for every shape and never falls back."""
    dev, seed = torch.device("cuda", torch.cuda.current_device()), _seed(seed)
    deterministic = deterministic or getattr(probs, "det", False)

    def post(k):                    # the workspace of this chunk's count
        ws = _ln_workspace(k, d, dev, "bpm_ln_bwd_det_ws_bytes") if deterministic else _ln_workspace(k, d, dev)
        return d, seed, ws.data_ptr(), ws.numel() * 4
    try:
        _grouped("bpm_ln_bwd_det" if deterministic else "bpm_ln_bwd_ws", probs, (BPM_F32 if dtype is None else dtype,), post)
    except RuntimeError:
        _LN_WS.clear()              # an aborted launch may leave ticket words set: start from fresh zeroed workspaces
        raise


def cast_problem(a, lda, R, Cn, *, a_is_ct=False, b=None, ldb=0, dst_ct=None, ldd=0, ct_cols=0, dst_f32=None, ldf=0, colsum=None,
                 drop_p=0.0, drop_site=0) -> CastProblem:
    p = CastProblem()
    p.a, p.lda, p.a_is_ct = _p(a), lda, int(a_is_ct)
    p.b, p.ldb = _f32(b, "cast.b"), ldb
    p.dst_ct, p.ldd, p.ct_cols, p.dst_f32, p.ldf = _p(dst_ct), ldd, ct_cols, _f32(dst_f32, "cast.dst_f32"), ldf
    p.colsum = colsum if isinstance(colsum, int) else _f32(colsum, "cast.colsum")
    p.R, p.C, p.drop_p, p.drop_site = R, Cn, drop_p, drop_site
    return p


def rows_cast(dtype, probs, seed=0) -> None:
    _grouped("bpm_rows_cast", probs, (dtype,), (_seed(seed),))


_CAST_WS = {}


def rows_cast_ws(dtype, probs, seed=0) -> None:
    """rows_cast with its column sums through a per-(device, stream) partial-row workspace and a finishing launch
    instead of float atomics (bpm_rows_cast_ws, deterministic mode)."""
    L, s, seed = _lib.lib(), _stream(), _seed(seed)
    arr = _as_array(CastProblem, probs)
    dev = torch.device("cuda", torch.cuda.current_device())
    for i in range(0, len(arr), MAX_GROUP):
        k = min(MAX_GROUP, len(arr) - i)
        need = L.bpm_rows_cast_ws_bytes(_at(arr, i), k)
        ws = _CAST_WS.get((str(dev), s))
        if ws is None or ws.numel() * 4 < need:
            if ws is not None:
                _WS_RETIRED.append(ws)          # a captured graph may still hold its address
            ws = _CAST_WS[(str(dev), s)] = torch.zeros((need + 3) // 4, device=dev, dtype=torch.float32)
        _lib.check(L.bpm_rows_cast_ws(dtype, _at(arr, i), k, seed, ws.data_ptr(), ws.numel() * 4, s), "bpm_rows_cast_ws")


def gelu_problem(u, ldu, R, Cn, *, u_is_ct=False, g=None, ldg=0, dg=None, lddg=0, du=None, lddu=0) -> "_lib.GeluProblem":
    """Exact (erf) GELU rows: forward g (CT [R, ldg], pad zeroed) = gelu(u); backward du (CT [R, lddu]) = dg * gelu'(u),
    dg fp32 [R, lddg].  u is fp32 or (u_is_ct) CT [R, ldu]."""
    p = _lib.GeluProblem()
    p.u, p.ldu, p.u_is_ct = _p(u), ldu, int(u_is_ct)
    p.g, p.ldg, p.dg, p.lddg, p.du, p.lddu = _p(g), ldg, _f32(dg, "gelu.dg"), lddg, _p(du), lddu
    p.R, p.C = R, Cn
    return p


def gelu_fwd(dtype: int, probs) -> None:
    _grouped("bpm_gelu_fwd", probs, (dtype,))


def gelu_bwd(dtype: int, probs) -> None:
    _grouped("bpm_gelu_bwd", probs, (dtype,))


def _ids(t, what: str, B: int, L: int):
    if t is None:
        return None
    if t.dtype != torch.int64 or tuple(t.shape) != (B, L) or not t.is_contiguous():
        raise ValueError(f"{what}: a contiguous int64 [B, L] tensor")
    return _p(t)


def bert_embed_problem(ids, seg, word, pos, typ, gamma, beta, *, x, s, mean, rstd, bad, xc=None, ldc: int = 0, drop_p: float = 0.0,
                       drop_site: int = 0) -> "_lib.BertEmbedProblem":
    """bpm_bert_embed_fwd: ids / seg int64 [B, L] (seg None = all zeros), the three fp32 tables [rows, d] (views with
    contiguous rows are fine), outputs in time-major rows (t*B + b); bad: the int32 device counter of ids outside a table."""
    B, L = ids.shape
    d = word.shape[1]
    p = _lib.BertEmbedProblem()
    p.ids, p.seg = _ids(ids, "bert_embed.ids", B, L), _ids(seg, "bert_embed.seg", B, L)
    p.word, p.pos, p.type = _f32_table(word, "bert_embed.word", d), _f32_table(pos, "bert_embed.pos", d), _f32_table(typ, "bert_embed.type", d)
    p.V, p.P, p.Tt = word.shape[0], pos.shape[0], typ.shape[0]
    p.gamma, p.beta, p.B, p.L = _f32(gamma, "bert_embed.gamma"), _f32(beta, "bert_embed.beta"), B, L
    p.x, p.xc, p.ldc = _f32(x, "bert_embed.x"), _p(xc), ldc
    p.s, p.mean, p.rstd = _f32(s, "bert_embed.s"), _f32(mean, "bert_embed.mean"), _f32(rstd, "bert_embed.rstd")
    p.bad, p.drop_p, p.drop_site = _counter(bad, "bert_embed.bad"), drop_p, drop_site
    return p


def bert_embed_fwd(dtype: int, prob, d: int, eps: float, seed: int = 0) -> None:
    _lib.check(_lib.lib().bpm_bert_embed_fwd(dtype, C.byref(prob), d, eps, _seed(seed), _stream()), "bpm_bert_embed_fwd")


def bert_embed_scatter_ws_bytes(rows: int, d: int, type_rows: int) -> int:
    return int(_lib.lib().bpm_bert_embed_scatter_ws_bytes(rows, d, type_rows))


def bert_scatter_problem(ds, B: int, L: int, ws, *, sorted_ids=None, perm=None, seg=None, dword=None, padding_idx=None, dpos=None,
                         dtype_=None) -> "_lib.BertScatterProblem":
    """bpm_bert_embed_scatter: ds fp32 [L*B, d] time-major; dword (zeroed by the caller) needs sorted_ids / perm = the stable
    sort of ids.view(-1); a gradient left None is not computed."""
    p = _lib.BertScatterProblem()
    p.ds, p.B, p.L = _f32(ds, "bert_scatter.ds"), B, L
    for t, what in ((sorted_ids, "sorted_ids"), (perm, "perm")):
        if t is not None and (t.dtype != torch.int64 or t.numel() != B * L or not t.is_contiguous()):
            raise ValueError(f"bert_scatter.{what}: a contiguous int64 tensor of B*L elements")
    p.sorted_ids, p.perm, p.seg = _p(sorted_ids), _p(perm), _ids(seg, "bert_scatter.seg", B, L)
    p.dword, p.dpos, p.dtype = _f32(dword, "bert_scatter.dword"), _f32(dpos, "bert_scatter.dpos"), _f32(dtype_, "bert_scatter.dtype")
    p.V = dword.shape[0] if dword is not None else 0
    p.Tt = dtype_.shape[0] if dtype_ is not None else 0
    if dpos is not None and dpos.shape[0] < L:
        raise ValueError("bert_scatter.dpos: fewer rows than time steps")
    p.padding_idx = -1 if padding_idx is None else int(padding_idx)
    p.ws, p.ws_bytes = _f32(ws, "bert_scatter.ws"), (ws.numel() * 4 if ws is not None else 0)
    return p


def bert_embed_scatter(prob, d: int) -> None:
    _lib.check(_lib.lib().bpm_bert_embed_scatter(C.byref(prob), d, _stream()), "bpm_bert_embed_scatter")


def loss_ws_bytes(kind: int, reduction: int, B: int, Cn: int) -> int:
    return int(_lib.lib().bpm_loss_ws_bytes(kind, reduction, B, Cn))


def loss_problem(kind: int, reduction: int, logits, target, loss, B: int, Cn: int, *, ld: Optional[int] = None, ldt: Optional[int] = None,
                 weight=None, ignore_index: int = -100, dlogits_unit=None, ldd: Optional[int] = None, bad=None, ws=None) -> "_lib.LossDesc":
    """bpm_loss_fwd / bpm_loss_bwd: logits fp32 [B, ld], target fp32 [B, ldt] (LOSS_BCE, LOSS_L1) or int64 [B] (LOSS_CE),
    weight fp32 [C] (pos_weight / class weight), loss fp32 (one value, or the elements / rows for LOSS_NONE), dlogits_unit
    fp32 [B, ldd] or None (no derivative wanted), bad: the int32 device counter of class indices outside [0, C), ws: any
    tensor of at least loss_ws_bytes(...) bytes.  Leading dimensions default to C."""
    p = _lib.LossDesc()
    p.kind, p.reduction, p.B, p.C = kind, reduction, B, Cn
    p.logits, p.ld = _f32(logits, "loss.logits"), Cn if ld is None else ld
    if kind == _lib.LOSS_CE:
        if target is not None and not isinstance(target, int) and target.dtype != torch.int64:
            raise ValueError(f"loss.target: cross-entropy takes int64 class indices, got {target.dtype}")
        p.target, p.ldt = _p(target), 0
    else:
        p.target, p.ldt = _f32(target, "loss.target"), Cn if ldt is None else ldt
    p.weight, p.ignore_index, p.loss = _f32(weight, "loss.weight"), ignore_index, _f32(loss, "loss.loss")
    p.dlogits_unit, p.ldd = _f32(dlogits_unit, "loss.dlogits_unit"), Cn if ldd is None else ldd
    p.bad = _counter(bad, "loss.bad")
    p.ws, p.ws_bytes = _p(ws), (ws.numel() * ws.element_size() if ws is not None else 0)
    return p


def loss_fwd(prob) -> None:
    _lib.check(_lib.lib().bpm_loss_fwd(C.byref(prob), _stream()), "bpm_loss_fwd")


def loss_bwd(prob, g, dlogits, *, ldg: Optional[int] = None, lddl: Optional[int] = None) -> None:
    """dlogits = prob.dlogits_unit * g; g: one fp32 device value (mean / sum) or the elements / rows (LOSS_NONE), read by
    the kernel when it runs."""
    _lib.check(_lib.lib().bpm_loss_bwd(C.byref(prob), _f32(g, "loss.g"), prob.C if ldg is None else ldg, _f32(dlogits, "loss.dlogits"),
                                       prob.C if lddl is None else lddl, _stream()), "bpm_loss_bwd")


def eval_ws_bytes(kind: int, capacity: int, Cn: int) -> int:
    return int(_lib.lib().bpm_eval_ws_bytes(kind, capacity, Cn))


def _bytes(t, what):
    if t is not None and not isinstance(t, int) and t.dtype != torch.uint8:
        raise ValueError(f"{what}: expected uint8, got {t.dtype}")
    return _p(t)


def eval_desc(kind: int, Cn: int, capacity: int, *, max_batches: int = 0, score=None, predict=None, raw=None, target=None,
              pred=None, label=None, losses=None, bad=None, result=None, counts=None, ws=None) -> "_lib.EvalDesc":
    """The store and outputs of bpm_eval_update / bpm_eval_finalize (include/bpmult_hip.h): fp32 score / predict / raw /
    target, uint8 pred / label, fp32 losses [max_batches], the int32 counter `bad`, fp64 result, int64 counts, ws: any
    tensor of at least eval_ws_bytes(...) bytes.  The per-call fields are set by eval_update / eval_finalize."""
    p = _lib.EvalDesc()
    p.kind, p.C, p.capacity, p.max_batches = kind, Cn, capacity, max_batches
    p.score, p.predict, p.raw = _f32(score, "eval.score"), _f32(predict, "eval.predict"), _f32(raw, "eval.raw")
    p.target, p.losses = _f32(target, "eval.target"), _f32(losses, "eval.losses")
    p.pred, p.label = _bytes(pred, "eval.pred"), _bytes(label, "eval.label")
    p.bad = _counter(bad, "eval.bad")
    if result is not None and not isinstance(result, int) and result.dtype != torch.float64:
        raise ValueError(f"eval.result: expected float64, got {result.dtype}")
    if counts is not None and not isinstance(counts, int) and counts.dtype != torch.int64:
        raise ValueError(f"eval.counts: expected int64, got {counts.dtype}")
    p.result, p.counts = _p(result), _p(counts)
    p.ws, p.ws_bytes = _p(ws), (ws.numel() * ws.element_size() if ws is not None else 0)
    return p


def eval_update(desc, logits, targets, B: int, n0: int, *, ld: Optional[int] = None, ldt: Optional[int] = None, loss=None,
                batch_index: int = 0) -> None:
    """Append rows [n0, n0 + B): logits fp32 [B, ld], targets fp32 [B, ldt] (multilabel), fp32 [B] (regression) or int64 [B]
    (classes); loss: a device fp32 scalar copied to losses[batch_index].  One launch, no host read."""
    desc.logits, desc.ld = _f32(logits, "eval.logits"), desc.C if ld is None else ld
    if desc.kind == _lib.EVAL_CLASSES:
        if targets is not None and not isinstance(targets, int) and targets.dtype != torch.int64:
            raise ValueError(f"eval.targets: class indices are int64, got {targets.dtype}")
        desc.targets, desc.ldt = _p(targets), 0
    else:
        desc.targets, desc.ldt = _f32(targets, "eval.targets"), desc.C if ldt is None else ldt
    desc.loss, desc.B, desc.n0, desc.batch_index = _f32(loss, "eval.loss"), B, n0, batch_index
    _lib.check(_lib.lib().bpm_eval_update(C.byref(desc), _stream()), "bpm_eval_update")


def eval_finalize(desc, N: int, nbatches: int) -> None:
    desc.N, desc.nbatches = N, nbatches
    _lib.check(_lib.lib().bpm_eval_finalize(C.byref(desc), _stream()), "bpm_eval_finalize")


def eval_image_bytes(kind: int, rows: int, batches: int, Cn: int) -> int:
    """Bytes of the exchange image of a shard of up to `rows` rows and `batches` losses (0: arguments not accepted)."""
    return int(_lib.lib().bpm_eval_image_bytes(kind, rows, batches, Cn))


def _image(t, what):
    if t.dtype != torch.int32 or not t.is_contiguous():
        raise ValueError(f"{what}: expected contiguous int32, got {t.dtype} with strides {t.stride()}")
    return _p(t)


def eval_pack(desc, n: int, nb: int, image, *, rows: Optional[int] = None, batches: Optional[int] = None) -> None:
    """Rows [0, n), losses [0, nb) and the bad counter of desc's store into `image` (int32, every word written, zero past
    the shard's data), laid out for (rows, batches): default (n, nb).  One launch, no host read."""
    _lib.check(_lib.lib().bpm_eval_pack(C.byref(desc), n, nb, n if rows is None else rows, nb if batches is None else batches,
                                        _image(image, "eval.image"), image.numel() * 4, _stream()), "bpm_eval_pack")


def eval_merge(desc, images, rows, batches) -> None:
    """images int32 [W, words], each laid out for (max(rows), max(batches)): rank r's rows to row sum(rows[:r]) of desc's
    store, its losses to batch sum(batches[:r]), bad = the sum of the images' counters.  One launch, no host read."""
    W = len(rows)
    if images.dim() != 2 or images.shape[0] != W or len(batches) != W:
        raise ValueError(f"eval.images: expected [W = {W}, words] and {W} batch counts, got {tuple(images.shape)} and {len(batches)}")
    arr = C.c_int * W
    _lib.check(_lib.lib().bpm_eval_merge(C.byref(desc), _image(images, "eval.images"), images.shape[1] * 4, W, arr(*rows), arr(*batches),
                                         _stream()), "bpm_eval_merge")


def addn_problem(out, ins) -> "_lib.AddnProblem":
    """out = sum(ins): contiguous fp32 tensors of one size (16-byte aligned); out may be one of them."""
    p = _lib.AddnProblem()
    n = out.numel()
    if not 1 <= len(ins) <= 8:
        raise ValueError("add_n takes 1 to 8 inputs")
    for t in (out, *ins):
        if t.dtype != torch.float32 or t.numel() != n or not t.is_contiguous():
            raise ValueError("add_n: contiguous float32 tensors of one size")
    p.out, p.n_in, p.count = _p(out), len(ins), n
    for j, t in enumerate(ins):
        p.src[j] = _p(t)
    return p


def expand_problem(q, dO, qexp, dOexp, B, H, T, dh, dhp, ld, *, Pd=None, S=0, dbias=None) -> "_lib.ExpandProblem":
    """bpm_expand_heads: head-major q / dO [B,H,T,dhp] -> block rows [(h*T+t)*B+b, ld]; dbias[H*dh] (written) =
    sum_{b,t} rowsum(Pd row) * dO[b,h,t,:]."""
    p = _lib.ExpandProblem()
    p.q, p.dO, p.qexp, p.dOexp, p.Pd, p.dbias = _p(q), _p(dO), _p(qexp), _p(dOexp), _p(Pd), _f32(dbias, "expand.dbias")
    p.B, p.H, p.T, p.S, p.dh, p.dhp, p.ld = B, H, T, S, dh, dhp, ld
    return p


def expand_heads(dtype: int, probs) -> None:
    _grouped("bpm_expand_heads", probs, (dtype,))


def add_n(probs) -> None:
    _grouped("bpm_add_n", probs)


def gmu_problem(a1, a2, ag, x1, x2, R, *, out=None, dout=None, da1=None, da2=None, dag=None, ldg=0, dx1=None, dx2=None) -> GmuProblem:
    p = GmuProblem()
    p.a1, p.a2, p.ag, p.x1, p.x2 = (_f32(t, "gmu") for t in (a1, a2, ag, x1, x2))
    p.out, p.dout = _f32(out, "gmu.out"), _f32(dout, "gmu.dout")
    p.da1, p.da2, p.dag, p.ldg = _p(da1), _p(da2), _p(dag), ldg
    p.dx1, p.dx2, p.R = _f32(dx1, "gmu.dx1"), _f32(dx2, "gmu.dx2"), R
    return p


def gmu2_fwd(probs, d) -> None:
    _grouped("bpm_gmu2_fwd", probs, (), (d,))


def gmu2_bwd(dtype, probs, d) -> None:
    _grouped("bpm_gmu2_bwd", probs, (dtype,), (d,))


# ----------------------------------------------------------------------------
# [B,d] tail: token pick + n-way gated fusion + residual head
# ----------------------------------------------------------------------------
def tail_fwd(desc, seed: int = 0) -> None:
    _lib.check(_lib.lib().bpm_tail_fwd(C.byref(desc), _seed(seed), _stream()), "bpm_tail_fwd")


def tail_bwd(desc, grads) -> None:
    _lib.check(_lib.lib().bpm_tail_bwd(C.byref(desc), C.byref(grads), _stream()), "bpm_tail_bwd")


# ----------------------------------------------------------------------------
# launch-table steps: (fn, *args), run as fn(*args, seed=seed) if fn is in SEEDED, else as fn(*args)
# ----------------------------------------------------------------------------
# every launch function above that takes a dropout seed: as the keyword `seed`
SEEDED = frozenset({gemm_grouped, attn_fwd, attn_bwd, attn_bwd_dq, attn_bwd_dkv, attn_fwd_kmask, attn_bwd_dq_kmask, attn_bwd_dkv_kmask,
                    pack_rows_fwd, pack_rows_bwd, embed_pos_fwd, embed_pos_bwd, kv_source_fwd, kv_source_bwd, ln_bwd, rows_cast,
                    bert_embed_fwd, tail_fwd})
# every function that may stand in a step table: a launch on the current stream with no result
# (the *_amask attention entries are called directly by models/attention.py and stand in no table)
STEP_FUNCTIONS = SEEDED | {attn_maps, ln_fwd, gelu_fwd, gelu_bwd, expand_heads, add_n, gmu2_fwd, gmu2_bwd, pack_weights, fold_bias,
                           unfold_grads, unfold_grads_ws, zero_segments}
