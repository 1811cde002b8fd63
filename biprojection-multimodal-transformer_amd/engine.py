"""Host-side orchestration of the BPMulT hot path on one MI355X.

Nothing here computes: it owns device buffers (allocated through torch), builds
the per-layer problem tables once per batch shape, and replays them through the
C ABI (ops.py) in forward and in a hand-ordered backward.  The design follows
the hardware, not the reference's call order:

* ParamStore -- every trunk parameter is a view into ONE flat fp32 master
  buffer, its gradient a view into ONE flat fp32 gradient buffer (what the
  RCCL all-reduce buckets and a fused optimizer want), and every 2-D weight has
  a CT (f32 / bf16) "shadow" with a 32-padded leading dimension, refreshed by a
  single table-driven launch per step.
* EncoderGroupPlan -- the independent encoders of one level (six in BPMulT,
  SURVEY.md 3.2) advance layer by layer in lock-step; every kernel launch of a
  layer serves all of them (grouped GEMM / attention / row kernels), so small
  per-encoder problems still fill 256 CUs and launches drop 6x.
* Activations needed by backward are kept in per-layer buffers in the layout
  the backward GEMMs consume (CT row-major for wgrad operands, head-major for
  attention); the [T,S] attention matrix is never stored (only row LSE).

Reference semantics implemented (file:line): transformer.py:52-93 (encoder),
141-195 (layer variants), multihead_attention.py:52-135, mmtr.py:189-195 (GMU).
"""
from __future__ import annotations

import ctypes as C
import math
import os
from collections import defaultdict
from dataclasses import dataclass
from typing import Dict, List, NamedTuple, Optional, Sequence, Tuple

import torch

from . import ops
from ._lib import (BPM_BF16, AdamSeg, adam_set_group, AddnProblem, ExpandProblem, F_CT_NARROW, F_ACCUM, F_BACKGROUND, F_KPAD, F_RELU, GEMM_NN, GEMM_NT, GEMM_TN, OUT_CT, OUT_HEADS,
                   AttnProblem, CastProblem, FoldDesc, GemmProblem, KvSourceProblem, LnProblem, PackDesc,
                   UnfoldDesc)
from .ops import pad32

# dropout site ids (unique per encoder / layer / op; the seed changes per step)
S_EMB_Q, S_EMB_K, S_EMB_V, S_ATTN, S_RES1, S_RELU, S_RES2, S_ATTN_SELF, S_RES0 = range(9)
SITE_TEXT = 1 << 20


def site(enc_id: int, layer: int, op: int) -> int:
    return (enc_id << 12) | (layer << 4) | op


def dhp_for(dh: int) -> int:
    if dh <= 32:
        return 32
    if dh <= 64:
        return 64
    if dh <= 128:
        return 128
    if dh <= 256:
        return 256
    raise ValueError(f"head_dim {dh} > 256 is not supported by the attention kernels (limit 256)")


_TABLES: Dict[Tuple[int, int, str], torch.Tensor] = {}


def sinusoid_table(n_pos: int, d: int, device) -> torch.Tensor:
    """fp32 [n_pos, d] table of position_embedding.py:44-60, built once on the
    host with the same torch CPU ops as the reference (bit-identical rows) and
    kept resident on the device."""
    key = (d, str(device))
    t = _TABLES.get(key)
    if t is None or t.shape[0] < n_pos:
        n = max(n_pos, 513)
        half = d // 2
        step = math.log(10000.0) / (half - 1)
        freq = torch.exp(torch.arange(half, dtype=torch.float32) * -step)
        ang = torch.arange(n, dtype=torch.float32)[:, None] * freq[None, :]
        tab = torch.cat([ang.sin(), ang.cos()], dim=1)
        if d % 2 == 1:
            tab = torch.cat([tab, torch.zeros(n, 1)], dim=1)
        tab[0].zero_()
        t = tab.contiguous().to(device)
        _TABLES[key] = t
    return t


# ----------------------------------------------------------------------------
# parameters
# ----------------------------------------------------------------------------
class ParamStore:
    """Flat fp32 master + gradient buffers and CT weight shadows for a set of
    nn.Parameters (all on one CUDA device)."""

    ALIGN = 64  # elements

    def __init__(self, named_params: Sequence[Tuple[str, torch.nn.Parameter]], dtype: int, x3: bool = False):
        self._dirty, self._dirty_rest, self._shadow_sig = True, False, None
        self._zero_table = None                         # built by set_store_written()
        self.dtype = dtype
        self.x3 = bool(x3) and dtype != BPM_BF16      # bf16x3 mode: fp32 storage, large GEMMs as three split-bf16 products
        self.side_low = True                            # side-stream priority: set by the plan that launches over this store
        self.names = [n for n, _ in named_params]
        self.params = {n: p for n, p in named_params}
        dev = named_params[0][1].device
        if dev.type != "cuda" and not ops._DRY_RUN:
            raise RuntimeError("BPMulT hot path: parameters must live on a CUDA (HIP) device; there is no CPU path")
        self.device = dev
        self.x3_cache = ops.X3Cache(dev) if self.x3 else None       # split images of the weight shadows: they go with the store
        self.off: Dict[str, int] = {}
        total = 0
        for n, p in named_params:
            self.off[n] = total
            total += (p.numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
        self.total = total
        self.master = torch.zeros(total, device=dev, dtype=torch.float32)
        self.gflat = torch.zeros(total, device=dev, dtype=torch.float32)
        with torch.no_grad():
            for n, p in named_params:
                v = self.master[self.off[n]: self.off[n] + p.numel()].view(p.shape)
                v.copy_(p.data)
                p.data = v
        self._gviews = {n: self.gflat[self.off[n]: self.off[n] + p.numel()].view(p.shape) for n, p in named_params}
        self._shadow_specs: List[Tuple[str, int, int, int, int, int, int, int]] = []
        self._shadow_off: Dict[str, int] = {}
        self._shadow_total = 0
        self._fold_specs: List[tuple] = []
        self._fold_off: Dict[str, int] = {}
        self._fold_total = 0
        self._fold_table = None
        self.shadow_flat: Optional[torch.Tensor] = None
        self._table = None
        self._norm_table = None                         # built by the first grad_sumsq()
        self._norm_set = None                           # (names, table, workspace, result) of the first grad_sumsq(names=...)
        self._master_ptr = self.master.data_ptr()

    # -- masters / grads ------------------------------------------------------
    def p(self, name: str) -> torch.Tensor:
        return self.params[name].data

    def g(self, name: str) -> torch.Tensor:
        return self._gviews[name]

    def gptr(self, name: str, elem_off: int = 0) -> int:
        return self._gviews[name].data_ptr() + 4 * elem_off

    def still_flat(self) -> bool:
        """False after anything re-pointed a parameter's storage (model.to()/.cuda()/.float(), `p.data = ...`, a
        child module that built a ParamStore of its own): the launch tables cache raw pointers into `master`, so
        every parameter is checked (~1700 integer comparisons)."""
        base = self._master_ptr
        return all(p.data_ptr() == base + 4 * self.off[n] for n, p in self.params.items())

    def _fresh(self) -> bool:
        """Gradients are unset (backward starts from zero) iff the first TRAINABLE parameter has no .grad: a frozen
        first parameter never gets one and must not make every micro-step look fresh."""
        for n in self.names:
            p = self.params[n]
            if p.requires_grad:
                return p.grad is None
        return True

    def set_store_written(self, names) -> None:
        """`names`: the parameters whose gradient the backward launch tables WRITE (plain store by their first
        weight-gradient launch of a step) when the gradients start from zero -- the large encoder matrices.  Everything
        else (biases, LayerNorm affines, Fusion-GMU / projection / unused parameters: sums of several launches, or
        never written) is what begin_backward(stores=True) clears, through one table-driven launch."""
        skip = set(names)
        segs, cur = [], None
        for n in self.names:                               # flat order: runs of consecutive other parameters (padding included)
            a, b = self.off[n], self.off[n] + self.params[n].numel()
            if n in skip:
                if cur is not None:
                    segs.append(tuple(cur))
                cur = None
            elif cur is None:
                cur = [a, b]
            else:
                cur[1] = b
        if cur is not None:
            segs.append(tuple(cur))
        base = self.gflat.data_ptr()
        self._zero_table = ops.zero_table([(base + 4 * a, b - a) for a, b in segs]) if segs else None
        self._store_written = skip

    def begin_backward(self, stores: bool = False) -> bool:
        """Gradients accumulate into gflat like autograd accumulates into .grad: a parameter whose .grad is None starts
        from zero.  stores=True (the caller's launch tables have a first-writer-stores variant, set_store_written): when
        the gradients are unset, only the small tensors are cleared and True is returned -- the caller must then run the
        storing tables."""
        fresh = self._fresh()
        if stores and fresh and self._zero_table is not None:
            ops.zero_segments(*self._zero_table)
            return True
        if fresh:
            self.gflat.zero_()
        return False

    def end_backward(self) -> None:
        for n in self.names:
            p = self.params[n]
            if p.grad is None and p.requires_grad:
                p.grad = self._gviews[n]

    # -- shadows --------------------------------------------------------------
    def add_shadow(self, key: str, name: str, rows: int, cols: int, *, src_col0: int = 0, src_ld: Optional[int] = None,
                   dst_ld: Optional[int] = None, dst_col0: int = 0, base_key: Optional[str] = None, src_row0: int = 0,
                   colscale: Optional[str] = None, dst_row0: int = 0) -> None:
        """Register a CT shadow [rows, dst_ld] of master `name` viewed as [.., src_ld][src_row0:src_row0+rows,
        src_col0:src_col0+cols].  base_key: write into an already registered shadow (block at row dst_row0, column
        dst_col0) instead of a new one.  colscale: name of a [cols] parameter multiplied into the columns (LayerNorm gain
        folding)."""
        ld = pad32(cols)
        src_ld = cols if src_ld is None else src_ld
        dst_ld = ld if dst_ld is None else dst_ld
        if base_key is None:
            self._shadow_off[key] = self._shadow_total
            off = self._shadow_total
            self._shadow_total += rows * dst_ld
        else:
            off = self._shadow_off[base_key] + dst_row0 * dst_ld
            self._shadow_off[key] = off + dst_col0
        self._shadow_specs.append((name, rows, cols, ld, src_ld, dst_ld, src_col0 + src_row0 * src_ld, off + dst_col0, colscale))

    def add_blank_shadow(self, key: str, rows: int, ld: int) -> None:
        """Reserve a zero-filled CT region [rows, ld] that later add_shadow(base_key=key, ...) calls fill block by block."""
        self._shadow_off[key] = self._shadow_total
        self._shadow_total += rows * ld

    def add_fold(self, key: str, wname: str, row0: int, rows: int, cols: int, beta: str, bias: str, bias_off: int) -> None:
        """Register a folded bias out[rows] = bias[bias_off:] + W[row0:row0+rows, :cols] . beta (fp32)."""
        self._fold_off[key] = self._fold_total
        self._fold_specs.append((wname, row0, rows, cols, beta, bias, bias_off, self._fold_total))
        self._fold_total += (rows + 63) // 64 * 64

    def fold(self, key: str, elem_off: int, n: int) -> torch.Tensor:
        o = self._fold_off[key] + elem_off
        return self.fold_flat[o:o + n]

    def finalize_shadows(self) -> None:
        ct = ops.ct_torch(self.dtype)
        self.shadow_flat = torch.zeros(max(self._shadow_total, 32), device=self.device, dtype=ct)
        if self.x3:                                    # the weight shadows are the static operands of the bf16x3 products
            a = self.shadow_flat.data_ptr()
            self.x3_cache.add_static(a, a + self.shadow_flat.numel() * self.shadow_flat.element_size())
        self._table = self._pack_table(self._shadow_specs)
        self._build_adam_table()
        self.fold_flat = torch.zeros(max(self._fold_total, 64), device=self.device, dtype=torch.float32)
        fd, blk = [], 0
        for (wname, row0, rows, cols, beta, bias, bias_off, off) in self._fold_specs:
            w = self.params[wname]
            ldw = w.shape[1]
            f = FoldDesc()
            f.W = w.data_ptr() + 4 * row0 * ldw
            f.beta = self.params[beta].data_ptr()
            f.b = self.params[bias].data_ptr() + 4 * bias_off
            f.out = self.fold_flat.data_ptr() + 4 * off
            f.rows, f.cols, f.ldw, f.blk0 = rows, cols, ldw, blk
            blk += (rows + 3) // 4
            fd.append(f)
        self._nfold, self._fold_blk = len(fd), blk
        self._fold_table = ops.device_table(fd) if fd else None

    def _pack_table(self, specs):
        """(device table, descriptors, blocks) of a pack_weights launch over a list of shadow specs; None for an empty one."""
        esz = self.shadow_flat.element_size()
        descs, blk = [], 0
        for (name, rows, cols, ld, src_ld, dst_ld, src_off, off, colscale) in specs:
            d = PackDesc()
            d.src = self.params[name].data_ptr() + 4 * src_off
            d.dst = self.shadow_flat.data_ptr() + esz * off
            d.rows, d.cols, d.ld, d.src_ld, d.dst_ld, d.blk0 = rows, cols, ld, src_ld, dst_ld, blk
            d.colscale = self.params[colscale].data_ptr() if colscale else None
            blk += (rows * ld + 1023) // 1024
            descs.append(d)
        return (ops.device_table(descs), len(descs), blk) if descs else None

    def _build_adam_table(self) -> None:
        """Segment table of the fused optimizer step (every segment in group 0) and the pack table of what it leaves over.
        A shadow is written BY THE OPTIMIZER KERNEL when it is the plain CT copy of a whole parameter matrix (the large
        encoder matrices, the projections, the GMU hidden maps, the time maps); shadows that mix two parameters (the K / V
        projection weights with their LayerNorm gain folded in) or re-arrange columns (the x_gate halves) stay with a second,
        small pack_weights launch (`_rest_table`), as do the folded biases."""
        esz = 2 if self.dtype == BPM_BF16 else 4
        plain, rest = {}, []
        for spec in self._shadow_specs:
            (name, rows, cols, ld, src_ld, dst_ld, src_off, off, colscale) = spec
            p = self.params[name]
            if (colscale is None and src_off == 0 and src_ld == cols and rows * cols == p.numel() and cols % 4 == 0
                    and name not in plain and (off * esz) % 16 == 0 and dst_ld % 4 == 0):
                plain[name] = (rows, cols, dst_ld, off)
            else:
                rest.append(spec)
        self._rest_table = self._pack_table(rest)
        self._adam_plain = plain
        self._adam_table = self._adam_segments(None)

    def _adam_segments(self, group_of: Optional[Dict[str, int]], raw: bool = False):
        """(device table, segments, blocks) over [0, total) in flat order: one segment per parameter with a plain shadow,
        runs of consecutive parameters without one.  group_of (bpm_adam_step_groups): {parameter name: group index, or -1
        for a parameter that is not stepped}; a run is then cut wherever the group changes, so that a segment belongs to
        exactly one group.  A parameter's alignment padding rides with it; offsets are 64-element aligned, so every cut
        is 16-byte aligned.  None: every segment in group 0 (`_adam_table`).  raw: the AdamSeg list itself (adam_sets_table)."""
        esz = 2 if self.dtype == BPM_BF16 else 4
        plain = self._adam_plain
        nblk = ops.adam_blocks
        segs, blk, run = [], 0, None              # run = [off, end, group) of consecutive parameters without a plain shadow
        for n in self.names:
            a = self.off[n]
            b = a + (self.params[n].numel() + self.ALIGN - 1) // self.ALIGN * self.ALIGN
            gi = 0 if group_of is None else group_of[n]
            if n in plain:
                if run is not None:
                    segs.append((run[0], run[1], None, run[2]))
                    run = None
                segs.append((a, b, plain[n], gi))
            elif run is None or run[2] != gi:
                if run is not None:
                    segs.append((run[0], run[1], None, run[2]))
                run = [a, b, gi]
            else:
                run[1] = b
        if run is not None:
            segs.append((run[0], run[1], None, run[2]))
        assert segs and segs[0][0] == 0 and segs[-1][1] == self.total and all(x[1] == y[0] for x, y in zip(segs, segs[1:]))
        out = []
        for a, b, sh, gi in segs:
            sg = AdamSeg()
            sg.off4, sg.n4, sg.blk0, sg.group = a // 4, (b - a) // 4, blk, gi
            if sh is not None:
                rows, cols, dst_ld, off = sh
                sg.dst, sg.rows, sg.cols, sg.dst_ld = self.shadow_flat.data_ptr() + esz * off, rows, cols, dst_ld
            blk += nblk((b - a) // 4)
            out.append(sg)
        return (ops.device_table(out), len(out), blk) if not raw else out

    def adam_group_table(self, group_of: Dict[str, int]):
        """The grouped segment table (device table, segments, blocks) for {parameter name: group index or -1}; a name the
        map leaves out is not stepped.  Built on every call: the optimizer keeps it until its groups change."""
        return self._adam_segments({n: group_of.get(n, -1) for n in self.names})

    def _build_norm_table(self) -> None:
        """Segment table of the gradient-norm reduction (bpm_grad_sumsq), its workspace and its 2-float result, all
        allocated once (stable addresses).  The segments are the exact element ranges of the TRAINABLE parameters in
        gflat, merged where one ends where the next begins: the alignment padding between parameters is left out (nothing
        promises that a gradient launch never writes there), and so is a frozen parameter's slice, which the backward
        launches still fill.  Built at the first use, from requires_grad as it is then -- FusedAdam fixes its parameter
        list the same way -- so a store that never clips or reads the norm allocates nothing."""
        self._norm_table, self._norm_ws = self._norm_segments(lambda n: self.params[n].requires_grad)
        self._norm_out = torch.zeros(2, device=self.device, dtype=torch.float32)

    def norm_ranges(self, counts) -> List[Tuple[int, int]]:
        """[(device address, elements)] of the gradient slices of the parameters `counts(name)` admits, merged where one
        ends where the next begins (bpm_grad_sumsq takes absolute addresses: one table may span several stores)."""
        segs: List[List[int]] = []
        for n in self.names:
            if not counts(n):
                continue
            a, b = self.off[n], self.off[n] + self.params[n].numel()
            if segs and segs[-1][1] == a:
                segs[-1][1] = b
            else:
                segs.append([a, b])
        base = self.gflat.data_ptr()
        return [(base + 4 * a, b - a) for a, b in segs]

    def _norm_segments(self, counts):
        segs: List[List[int]] = []
        for n in self.names:
            if not counts(n):
                continue
            a, b = self.off[n], self.off[n] + self.params[n].numel()
            if segs and segs[-1][1] == a:
                segs[-1][1] = b
            else:
                segs.append([a, b])
        if not segs:
            raise RuntimeError("gradient norm: no trainable parameter in the flat buffers")
        base = self.gflat.data_ptr()
        table = ops.sumsq_table([(base + 4 * a, b - a) for a, b in segs])
        return table, torch.empty(ops.grad_sumsq_ws_bytes(table[2]) // 4, device=self.device, dtype=torch.float32)

    def grad_sumsq(self, grad_scale: float = 1.0, max_norm: float = 0.0, extra_sumsq: Optional[torch.Tensor] = None,
                   names: Optional[frozenset] = None) -> torch.Tensor:
        """The global gradient norm without leaving the device: one reduction over the trainable parameters' slices of
        gflat (+ a tiny fixed-order sum).  Returns the store's persistent result [total_norm, coef]:
        total_norm = grad_scale * sqrt(sum of squares + extra_sumsq), coef = min(1, max_norm / (total_norm + 1e-6)), or 1
        when max_norm <= 0 (the norm only).  The next call overwrites it.
        names: the parameters that count, instead of requires_grad as it was at the first use -- an optimizer with
        parameter groups passes the set it steps (a table, workspace and result of its own, rebuilt when the set changes)."""
        if names is None:
            if self._norm_table is None:
                self._build_norm_table()
            (tab, nseg, nblk), ws, out = self._norm_table, self._norm_ws, self._norm_out
        else:
            if self._norm_set is None or self._norm_set[0] != names:
                self._norm_set = (names,) + self._norm_segments(lambda n: n in names) + (
                    torch.zeros(2, device=self.device, dtype=torch.float32),)
            _, (tab, nseg, nblk), ws, out = self._norm_set
        ops.grad_sumsq(tab, nseg, nblk, ws, out, grad_scale, max_norm, extra_sumsq)
        return out

    def adam_step(self, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, lr, beta1, beta2, eps, weight_decay, step, grad_scale,
                  zero_grad: bool, scale_dev: Optional[torch.Tensor] = None) -> None:
        """adam_step_groups over the whole trunk (`_adam_table`) as one L2 group at the host's step number."""
        one = ops.adam_groups([dict(lr=lr, betas=(beta1, beta2), eps=eps, weight_decay=weight_decay, step=step)])
        self.adam_step_groups(exp_avg, exp_avg_sq, self._adam_table, one, grad_scale, zero_grad, scale_dev=scale_dev)

    def adam_step_groups(self, exp_avg: torch.Tensor, exp_avg_sq: torch.Tensor, table, groups, grad_scale,
                         zero_grad: bool, scale_dev: Optional[torch.Tensor] = None, norm_dev: Optional[torch.Tensor] = None,
                         steps_dev: Optional[torch.Tensor] = None, skipped_dev: Optional[torch.Tensor] = None) -> None:
        """One launch (bpm_adam_step_groups): torch.optim.Adam's update of the trunk parameters (flat master / gradient /
        moments) AND the CT shadows of the plain weight matrices, written from the updated values as they are stored.  What
        is left for the next forward's refresh_shadows is the small rest (K / V weights with the LayerNorm gain folded in,
        folded biases).  table = adam_group_table({parameter name: index into `groups`}) or `_adam_table`; groups =
        ops.adam_groups(...).  scale_dev: one device float multiplied into grad_scale by the kernel (the clip coefficient
        of grad_sumsq).  norm_dev: the step is skipped on the device when that norm is not finite.
        When a full refresh is pending (the masters were edited since the last one) it runs first, one extra pack_weights
        launch: this launch need not rewrite every plain shadow (a parameter that is not stepped, a skipped step).  The
        stored results are the same with or without it, and a training loop never pays it: its forward has refreshed."""
        tab, nseg, nblk = table
        sig = self.begin_adam_step()
        ops.adam_step_groups(self.dtype, tab, nseg, nblk, self.master, self.gflat, exp_avg, exp_avg_sq, groups, grad_scale,
                             zero_grad, scale_dev, norm_dev, steps_dev, skipped_dev)
        self.end_adam_step(sig)

    def begin_adam_step(self) -> int:
        """Before a fused optimizer launch over this store: the pending full shadow refresh, if any (see adam_step_groups).
        Returns the version signature end_adam_step() takes."""
        sig = self._versions()                             # (the launches go through raw pointers: no counter moves)
        if self._dirty or sig != self._shadow_sig:
            self.refresh_shadows()
        return sig

    def end_adam_step(self, sig: int) -> None:
        """After it: every plain shadow holds the CT image of its master; the rest (shadows that mix parameters, folded
        biases) is stale until the next refresh_shadows."""
        self._dirty, self._dirty_rest, self._shadow_sig = False, True, sig

    def sptr(self, key: str, elem_off: int = 0) -> int:
        return self.shadow_flat.data_ptr() + self.shadow_flat.element_size() * (self._shadow_off[key] + elem_off)

    def mark_dirty(self) -> None:
        """The master weights were changed through raw pointers (bpm_adam_step) or through a `p.data` alias (neither
        bumps a version counter torch lets us see): the CT shadows are stale.  Writers of `p.data` MUST call this."""
        self._dirty = True

    invalidate = mark_dirty

    def broadcast(self, src: int = 0, group=None) -> None:
        """Replicate rank `src`'s flat master on every rank (one message) and invalidate the shadows."""
        import torch.distributed as dist
        dist.broadcast(self.master, src, group=group)
        self.mark_dirty()

    def _versions(self) -> int:
        # in-place ops on a parameter bump p._version; in-place ops on the flat master itself (dist.broadcast(master),
        # master.mul_(..), EMA / averaging written on the master) bump master._version only
        return self.master._version + sum(p._version for p in self.params.values())

    def refresh_shadows(self, force: bool = False) -> None:
        """Re-derive the CT weight shadows and folded biases from the fp32 masters -- only when the masters changed
        since the last refresh (an optimizer step, load_state_dict, any in-place edit: torch's per-tensor version
        counters, or mark_dirty() for raw-pointer writers).  In a training loop that is once per optimizer step."""
        sig = self._versions()
        full = force or self._dirty or sig != self._shadow_sig
        if not full and not self._dirty_rest:
            return
        self._dirty, self._dirty_rest, self._shadow_sig = False, False, sig
        if full:
            if self._table is not None:
                ops.pack_weights(self.dtype, *self._table)
        elif self._rest_table is not None:         # after a fused optimizer step: it wrote the plain shadows itself
            ops.pack_weights(self.dtype, *self._rest_table)
        if self._fold_table is not None:
            ops.fold_bias(self._fold_table, self._nfold, self._fold_blk)
        if self.x3:
            self.x3_cache.refresh_static()         # split images of the shadows that just changed (outside any graph)


def adam_sets_table(stores: Sequence[ParamStore], group_ofs: Sequence[Dict[str, int]]):
    """One segment table over SEVERAL stores for adam_step_sets (bpm_adam_step_sets): store i is buffer set i, its segments
    are those of its own adam_group_table(group_ofs[i]) -- {parameter name: group index}, a name left out is not stepped --
    with offsets relative to that store, in store order, blocks numbered through.  All stores share one CT."""
    if len({st.dtype for st in stores}) != 1:
        raise ValueError("adam_sets_table: the stores of one launch share one CT (the kernel writes every shadow in it)")
    segs = []
    for si, (st, group_of) in enumerate(zip(stores, group_ofs)):
        for sg in st._adam_segments({n: group_of.get(n, -1) for n in st.names}, raw=True):
            sg.group = adam_set_group(si, sg.group)
            segs.append(sg)
    return ops.adam_sets_table(segs)


def adam_step_sets(stores: Sequence[ParamStore], table, sets, groups, grad_scale, zero_grad: bool,
                   scale_dev: Optional[torch.Tensor] = None, norm_dev: Optional[torch.Tensor] = None,
                   steps_dev: Optional[torch.Tensor] = None, skipped_dev: Optional[torch.Tensor] = None) -> None:
    """ParamStore.adam_step_groups over several stores in ONE launch: table = adam_sets_table(stores, ...), sets =
    ops.adam_sets([(st.master, st.gflat, exp_avg, exp_avg_sq) for st in stores]).  The device step counts and the skip
    decision are read once for all stores, and the counters advance once."""
    sigs = [st.begin_adam_step() for st in stores]
    ops.adam_step_sets(stores[0].dtype, table, sets, groups, grad_scale, zero_grad, scale_dev, norm_dev, steps_dev, skipped_dev)
    for st, sig in zip(stores, sigs):
        st.end_adam_step(sig)


# ----------------------------------------------------------------------------
# encoder group
# ----------------------------------------------------------------------------
@dataclass
class EncoderDesc:
    """One encoder of a lock-step group.  `prefix` selects its parameters in the
    ParamStore (reference state_dict names, e.g. 'trans_l_with_a.')."""
    prefix: str
    enc_id: int
    T: int
    S: int
    attn_dropout: float
    # the T query rows are rows q_pos0 + i*q_stride of a length-T_full sequence (a gathered subset: SURVEY A.10);
    # positions and the attention mask follow the ORIGINAL time steps
    q_pos0: int = 0
    q_stride: int = 1
    T_full: Optional[int] = None
    # biprojection encoders only: the consumer reads rows {0, T-1} of the output, and under the causal
    # self-attention a row never sees a later one, so the LAST layer's query side (self-attention queries, cross
    # attention, FFN) and the final LayerNorm run on those two rows; its self-attention keys / values and every
    # earlier layer stay dense.  The output is then [2, B, d].
    tail_rows: bool = False


@dataclass
class EncoderMasks:
    """Which padding masks the forward calls of one encoder of a plan carry (EncoderGroupPlan(masks=...)): the content
    comes with every forward call, the plan is built for their presence."""
    self_keys: bool = False       # [B, T]: padding rows of the query sequence, hidden as keys of the self-attention block
    cross_keys: bool = False      # [B, S]: padding rows of the key / value source, hidden as keys of the cross-attention block


@dataclass
class GroupCfg:
    d: int
    H: int
    layers: int
    relu_dropout: float
    res_dropout: float
    embed_dropout: float
    attn_mask: bool
    biprojection: bool
    # self-attention-only stack, the reference's forward(x) (transformer.py:81-85, 158-159): keys and values are projected
    # from the query rows' LayerNorm-0 output; no key / value source, no folded key / value state (EncoderGroupPlan._kv)
    self_only: bool = False


SIDE, JOIN, MARK, WAIT, SIDE2 = "side", "join", "mark", "wait", "side2"


class AttentionMap(NamedTuple):
    """One attention map (EncoderGroupPlan.attention_maps).  weights: fp32 [B, Tq, S] (head-averaged) or [B, H, Tq, S]
    (per_head=True), the caller's own tensor.  query_steps: None when the Tq rows are all T time steps of the encoder's
    query sequence, else the time step of each row (layers that only compute a few query rows: a gathered subset, or rows {0, T-1} of a tail_rows layer)."""
    weights: torch.Tensor
    query_steps: Optional[Tuple[int, ...]]
_SIDE = os.environ.get("BPMULT_SIDE", "1") != "0"
# dK/dV attention pass: "0" main stream, "1" side stream, "2" a third stream, "auto": side stream.
# dK / dV feed only side-stream work (weight gradients, key/value dgrad).  At hidden 768 the main stream is the longer one
# (41 ms against 23 in round 2) and the pass on the side stream saved ~4 ms.  At hidden 300 the side stream used to be the
# longer one (round 2: +1 ms/step with the pass there); since the dead-row schedule and the LDS-DMA kernel for its NT / NN
# products the main stream is (46 against 31 ms busy at batch 64): configs[1] 8.77 -> 8.60, configs[3] 50.1 -> 49.7 ms.
_DKV_SIDE_ENV = os.environ.get("BPMULT_DKV_SIDE", "auto")
_side_streams: Dict[Tuple[int, int, bool], "torch.cuda.Stream"] = {}
# Priority of the side stream: "low" (the dispatcher fills CUs from the main stream first), "normal", or "auto": low
# below hidden 512, normal from there on.  Measured on MI355X: at hidden 300 low wins (16.9 -> 16.6 ms/step); at hidden
# 768 every GEMM workgroup owns a CU for 50-300 us, the side stream's weight gradients are a third of the step's work,
# and starving them only lengthens the tail (37.97 ms/step low, 37.53 normal).
_SIDE_PRIORITY_ENV = os.environ.get("BPMULT_SIDE_PRIORITY", "auto")
# Low-rank key side for groups with a handful of query time steps (EncoderGroupPlan._lowrank; "0": dK / dV as everywhere else)
_LOWRANK = os.environ.get("BPMULT_LOWRANK", "1") != "0"
# (Measured in round 3 and removed: a side stream restricted to 160-224 CUs by hipExtStreamCreateWithCUMask, so that the
# main stream's row kernels never queue behind weight-gradient workgroups: 47-51 ms/step against 32.5.  Also without
# effect: d(LayerNorm output) written as bf16 by the data-gradient GEMMs and read as bf16 by the LayerNorm backward --
# 75 MB less per launch pair, 31.2 -> 31.3 ms/step.)


# Side streams that hold work the main stream has not waited for yet (handle -> stream).  Inside a graph capture every such
# fork must be joined back into the capturing stream before the capture ends -- an unjoined one invalidates the capture
# (and crashed inside hipStreamEndCapture in round 3 with a second stream pair).  _run() adds on SIDE / SIDE2 and clears on
# JOIN; the graph code checks that nothing is left (open_forks) before it lets a capture end.
_OPEN_FORKS: Dict[int, "torch.cuda.Stream"] = {}


def open_forks() -> List["torch.cuda.Stream"]:
    return list(_OPEN_FORKS.values())


def _side_stream(device, which: int = 1, low: bool = True) -> "torch.cuda.Stream":
    """Side streams per device, created through the C ABI (low: at the device's LOWEST priority)."""
    dev_i = device.index if device.index is not None else torch.cuda.current_device()
    if _SIDE_PRIORITY_ENV in ("low", "normal"):
        low = _SIDE_PRIORITY_ENV == "low"
    key = (dev_i, which, bool(low))
    if key not in _side_streams:
        from . import _lib
        out = C.c_void_p()
        with torch.cuda.device(dev_i):
            _lib.check(_lib.lib().bpm_stream_create(int(bool(low)), C.byref(out)), "bpm_stream_create")
        _side_streams[key] = torch.cuda.ExternalStream(out.value, device=torch.device("cuda", dev_i))
    return _side_streams[key]


# buffer keys of the self-attention block: its own in a self-only plan; beside the cross-attention block's (which owns
# qh / kh / vh / ao / lse / xmid / dy and the parity-buffered dao / delta) in the biprojection layer kind
_SELF_KEYS = dict(q="qh", k="kh", v="vh", o="ao", lse="lse", mid="xmid", dy="dy", dao="dao", delta="delta")
_BIP_SELF_KEYS = dict(q="qs", k="ks", v="vs", o="aos", lse="lses", mid="xmid0", dy="dy0", dao="dao0", delta="delta0")


class EncoderGroupPlan:
    """Buffers + launch tables for G encoders x L layers at batch size B.

    Three layer kinds, each a fixed sequence of blocks (transformer.py:141-195, normalize_before):
      self-only (GroupCfg.self_only)  self-attention + FFN
      crossmodal                      cross-attention + FFN
      biprojection                    self-attention + cross-attention + FFN
    The per-block builders below (_ln0_* / _self_attn_* / _cross_attn_* / _ffn_*) append one encoder's problems of one
    layer to that layer's launch lists; _build_fwd / _build_bwd wire their operands and order the launches per kind."""

    def __init__(self, store: ParamStore, cfg: GroupCfg, encs: Sequence[EncoderDesc], B: int, x3: "Optional[ops.X3Cache]" = None,
                 masks: "Optional[Sequence[Optional[EncoderMasks]]]" = None, deterministic: Optional[bool] = None):
        self.store, self.cfg, self.encs, self.B = store, cfg, list(encs), B
        # DETERMINISTIC MODE (None: config.deterministic(), read HERE, where the tables are built -- a captured graph
        # carries the mode it was captured in).  The backward tables then hold no launch that adds floats in hardware
        # order ("Deterministic mode"): fc1.bias / fc2.bias / out_proj.bias ride on their weight-gradient
        # products (_bias_route), unfold_grads and the LayerNorm backward go through their workspace entries.
        from . import config
        self.det = config.resolve_deterministic(deterministic)
        # PADDING MASKS (masks[e]: which key masks encoder e's forward calls carry; None / all-False everywhere: an unmasked
        # plan, whose tables are what they always were).  A masked plan runs EVERY attention step through the *_kmask
        # entries, one mask per problem: the plan owns one visibility buffer per encoder and attention block (_alloc: vis_s
        # [B, T], vis_c [B, S]; uint8, nonzero = VISIBLE, the kernels' convention), the bpm_attn_kmask arrays below point at
        # them for the plan's life, and forward() refills them from the caller's masks -- the tables stay fixed while the
        # mask content changes from call to call.  A block that was given no mask keeps its buffer of ones.
        self.masks = [EncoderMasks() if m is None else m for m in (masks if masks is not None else [None] * len(self.encs))]
        if len(self.masks) != len(self.encs):
            raise ValueError(f"masks: one entry per encoder ({len(self.encs)} encoders, {len(self.masks)} entries)")
        self._masked = any(m.self_keys or m.cross_keys for m in self.masks)
        for e, m in zip(self.encs, self.masks):
            if m.self_keys and not (cfg.biprojection or cfg.self_only):
                raise ValueError(f"encoder {e.prefix}: a self-attention key mask, but the crossmodal layer kind has no self-attention block")
            if m.cross_keys and cfg.self_only:
                raise ValueError(f"encoder {e.prefix}: a cross-attention key mask, but a self-attention-only plan has no key / value source")
            if self._masked and (e.tail_rows or e.T_full is not None or e.q_pos0 or e.q_stride != 1):
                raise ValueError(f"encoder {e.prefix}: padding masks are not available with tail_rows or a gathered query subset")
        # bf16x3 mode: the owner of the activations' split images -- the caller's (a trunk shares one between its plans), or
        # this plan's own (a stand-alone encoder); the weight shadows' images stay with the store
        self.x3 = x3 if x3 is not None or not store.x3 else ops.X3Cache(store.device, weights=store.x3_cache)
        self.dtype = store.dtype
        d, H = cfg.d, cfg.H
        if d % H:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.dh = d // H
        self.dhp = dhp_for(self.dh)
        # key / value source: every kind but the self-attention-only stack, whose keys and values are projected from the
        # query rows' LayerNorm-0 output -- no key / value-side state, steps or unfold tables without one
        self._kv = not cfg.self_only
        # LOW-RANK KEY SIDE.  With T query time steps dK = dS^T Q and dV = Pd^T dO have rank T per (batch element, head), and
        # every key / value-side product of the backward factors through the [H T, S] matrices dS, Pd (written by the dQ
        # pass) instead of the [S B, d] matrices dK, dV:
        #   W_k' gradient  = Qexp^T (dS khat)           (was dK^T khat: d x d x S B -- now H T B x S x d, then d x d x H T B)
        #   d(khat)        = sum_layers dS^T (Qexp W_k') (was dK W_k' over K = layers d -- now K = layers H T)
        # and the same with Pd, dOexp, vhat, W_v' for the value side (Qexp / dOexp: the heads' vectors in their own column
        # block of otherwise-zero rows, bpm_expand_heads, so that all heads travel in one product).  Level 2 under dead-row
        # elimination has T = 2: at hidden 768 this removes 1.5 of the step's 19.4 ms (the key / value weight gradients over
        # 4096 rows, the merged K = 6144 data gradient, the dK / dV pass).  Equal to the dK / dV route in real arithmetic; the
        # roundings differ (dS instead of dK is rounded to CT), fixtures F7 / F9 / F11 hold both.  Crossmodal groups only.
        # Off in a masked plan: the masked dQ entries have no dS / Pd export (attention.hip, fill_masked).
        self._lowrank = (_LOWRANK and self._kv and not cfg.biprojection and not self._masked
                         and all(e.T * H * 4 <= d and e.S % 4 == 0 for e in self.encs) and self.dh <= 256)
        self.ld, self.ld4 = pad32(d), pad32(4 * d)
        self.scale = self.dh ** -0.5
        # KEY / VALUE SOURCES IN ONE PASS (bpm_kv_source_fwd / _bwd): embedding + affine-free LayerNorm of every key / value
        # source as one side-stream launch per direction, read from the caller's xk / xv -- no embedded copies (ke / ve) and
        # no LayerNorm-input gradients (dke / dve).  Same bits as the embed_pos / ln launches it replaces; BPMULT_KV_FUSED=0
        # (read when the plan is built) keeps those, as does a shape outside the kernels' domain.
        self._kv_fused = (self._kv and os.environ.get("BPMULT_KV_FUSED", "1") != "0"
                          and all(ops.kv_source_ok(d, e.S, B) for e in self.encs))
        self._kv_dst: List[Optional[torch.Tensor]] = [None] * len(self.encs)     # merge_kv_grads: where d(xk) + d(xv) goes
        self._kv_keep = None                                                     # the last forward's xk / xv (read again by backward)
        # FFN LayerNorm: layer_norms.2 in the biprojection kind (its layer_norms.1 normalises the key / value source, or is
        # the identity of maybe_layer_norm(1, after=True) in the self-attention-only stack: no gradient)
        self._lnF = 2 if cfg.biprojection else 1
        dev = store.device
        L = cfg.layers
        # accumulators that every backward starts from zero (d(khat), d(vhat), folded bias sums): ONE buffer, one fill
        nacc = sum(L * 2 * d + 16 for e in self.encs)
        self._acc0 = torch.zeros(nacc, device=dev, dtype=torch.float32)
        self._acc_off = 0
        self.buf: List[dict] = [self._alloc(e) for e in self.encs]
        # one bpm_attn_kmask per encoder and block, in encoder order like the problems of every attention launch
        self._km_self = self._km_cross = None
        if self._masked:
            if cfg.biprojection or not self._kv:
                self._km_self = ops.attn_kmasks([(b["vis_s"], e.T) for e, b in zip(self.encs, self.buf)])
            if self._kv:
                self._km_cross = ops.attn_kmasks([(b["vis_c"], e.S) for e, b in zip(self.encs, self.buf)])
        if cfg.biprojection and any(e.T_full is not None for e in self.encs):
            raise ValueError("a gathered query subset is only exact for crossmodal (non-biprojection) encoders")
        self.table = sinusoid_table(max(max(e.T_full or e.T, e.S) for e in self.encs) + 2, d, dev)
        self._ones, self._zeros = torch.ones(d, device=dev), torch.zeros(d, device=dev)
        # fused key / value sources: one problem per encoder, shared by the forward and the backward tables of a mode; the
        # source pointers are set by forward(), the gradient destinations by merge_kv_grads()
        self._kvsrc = {}
        if self._kv_fused:
            for training in (True, False):
                p = cfg.embed_dropout if training else 0.0
                self._kvsrc[training] = ops.array(KvSourceProblem, [
                    ops.kv_source_problem(None, None, e.S, B, khat=b["khat"], vhat=b["vhat"], ld=self.ld, stats_k=b["stk"],
                                          stats_v=b["stv"], gk=b["Gk"], gv=b["Gv"], dxk=b["dxk"], dxv=b["dxv"], drop_p=p,
                                          drop_site_k=site(e.enc_id, 0, S_EMB_K), drop_site_v=site(e.enc_id, 0, S_EMB_V))
                    for e, b in zip(self.encs, self.buf)])
        # table of the launch that turns folded K/V gradients into in_proj / LayerNorm parameter gradients
        lnK = 1 if cfg.biprojection else 0
        self._unfold = []                                  # one table per layer: its gradients are final with it
        for i in range(L if self._kv else 0):
            ud, blk = [], 0
            for e, b in zip(self.encs, self.buf):
                pn = lambda leaf: self._pn(e, i, leaf)
                u = UnfoldDesc()
                u.dWf, u.dbf = b["dWf"][i].data_ptr(), b["dbf"][i].data_ptr()
                u.W = store.p(pn("self_attn.in_proj_weight")).data_ptr() + 4 * d * d
                u.gamma, u.beta = store.p(pn(f"layer_norms.{lnK}.weight")).data_ptr(), store.p(pn(f"layer_norms.{lnK}.bias")).data_ptr()
                u.dW, u.dbias = store.gptr(pn("self_attn.in_proj_weight"), d * d), store.gptr(pn("self_attn.in_proj_bias"), d)
                u.dgamma, u.dbeta = store.gptr(pn(f"layer_norms.{lnK}.weight")), store.gptr(pn(f"layer_norms.{lnK}.bias"))
                u.rows, u.cols, u.ldw, u.blk0 = 2 * d, d, d, blk
                blk += (2 * d + 15) // 16
                ud.append(u)
            self._unfold.append((ops.device_table(ud), len(ud), blk))
        self._dkv_side = _DKV_SIDE_ENV if _DKV_SIDE_ENV != "auto" else "1"
        # a group whose query side is a handful of rows (level 2 under dead-row elimination) is bound by its SIDE stream
        # (key / value projections, their weight gradients): its dK / dV pass goes back to the main stream, which idles
        if _DKV_SIDE_ENV == "auto" and max(e.T for e in self.encs) * B <= 64:
            self._dkv_side = "0"
        self._side_low = d < 512
        self.store.side_low = self._side_low
        self._fwd = {True: self._build_fwd(True), False: self._build_fwd(False)}
        # Q / K / LSE of every layer hold one complete forward pass (attention_maps): cleared while a forward is being
        # launched, set when its last launch is enqueued (or its captured graph has been replayed: maps_ready)
        self._maps_ok = False
        # backward tables by (training, stores): stores = the first weight-gradient launch of each large matrix writes
        # instead of accumulating (the flat gradient buffer was not cleared: ParamStore.begin_backward(stores=True))
        self._bwd = {(t, f): self._build_bwd(t, f) for t in (True, False) for f in (True, False)}
        for steps in (*self._fwd.values(), *self._bwd.values()):
            self._check_steps(steps)
        if self.det:                      # no backward step of a deterministic plan may reach an entry that adds with atomics
            for steps in self._bwd.values():
                for s in steps:
                    s = s[1] if s is not JOIN and s[0] in (SIDE, SIDE2) else s
                    if s is not JOIN and s[0] is ops.ln_bwd and not getattr(s[1], "det", False):
                        raise ValueError("launch table: a LayerNorm-backward step of a deterministic plan is not marked (ops.ln_det)")
                    if s is not JOIN and s[0] is ops.unfold_grads:
                        raise ValueError("launch table: unfold_grads (float atomics) in a deterministic plan")

    def _alloc(self, e: EncoderDesc) -> dict:
        """Buffers of one encoder: the query chain and FFN of every kind, the self-attention block's (self-only and
        biprojection) and the cross-attention block's key / value-side state (kinds with a key / value source)."""
        c, B, d, H, L, ld, ld4, dhp = self.cfg, self.B, self.cfg.d, self.cfg.H, self.cfg.layers, self.ld, self.ld4, self.dhp
        dev, ct = self.store.device, ops.ct_torch(self.dtype)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
        if not self._kv and (e.S != e.T or e.tail_rows or e.T_full is not None or e.q_pos0 or e.q_stride != 1):
            raise ValueError(f"encoder {e.prefix}: a self-attention-only encoder attends over its own {e.T} time steps "
                             "(S == T, no gathered rows, no tail_rows)")
        has_self = c.biprojection or not self._kv
        R, Rk = e.T * B, e.S * B
        tailp = bool(e.tail_rows)
        if tailp and (not c.biprojection or e.T < 2 or e.T_full is not None):
            raise ValueError("tail_rows: biprojection encoders with at least two query rows (crossmodal encoders gather their rows)")
        # query-side rows / time steps of every layer (the last one shrinks to rows {0, T-1} with tail_rows)
        Rl, Tl = [R] * L, [e.T] * L
        if tailp:
            Rl[-1], Tl[-1] = 2 * B, 2
        b = dict(R=R, Rk=Rk, Rl=Rl, Tl=Tl, tailp=tailp)
        b["x"] = [z(R, d) for _ in range(L)] + [z(Rl[-1], d)]
        b["out"] = z(Tl[-1], B, d)
        b["stf"] = (z(Rl[-1]), z(Rl[-1]))
        if self._kv:
            if not self._kv_fused:
                b["ke"], b["ve"] = z(Rk, d), z(Rk, d)
            # key / value source, normalised ONCE without affine (the per-layer LayerNorm gain and bias are folded
            # into the K / V projection weights, see register_encoder_shadows)
            b["khat"], b["vhat"] = z(Rk, ld, dt=ct), z(Rk, ld, dt=ct)
            b["stk"], b["stv"] = (z(Rk), z(Rk)), (z(Rk), z(Rk))
            # d(khat), d(vhat) = sum over the layers of dK_i Wk'_i, dV_i Wv'_i: ONE product over K = L ld per encoder at the
            # end of backward (dK_i / dV_i of every layer are kept side by side in dkall / dvall) instead of L products
            # accumulating into the same fp32 [Rk, d] tensor (8 x 300 MB of read-modify-write per level at hidden 768)
            b["Gk"], b["Gv"] = z(Rk, d), z(Rk, d)
            if self._lowrank:
                HT, Sp = H * e.T, (e.S + 63) // 64 * 64
                b["Sp"] = Sp
                # dS / Pd of every layer, [layer][h*T + t][b][key] with zero key padding (never written); the same row
                # order (h*T + t)*B + b for the expanded head rows and everything computed from them
                b["dSall"], b["Pdall"] = z(L, HT, B, Sp, dt=ct), z(L, HT, B, Sp, dt=ct)
                b["qkall"], b["daall"] = z(L, HT * B, ld, dt=ct), z(L, HT * B, ld, dt=ct)
                for nm in ("qexp", "doexp", "U", "Av"):
                    b[nm] = [z(HT * B, ld, dt=ct) for _ in range(2)]
                b["dkall"] = b["dvall"] = None
            else:
                b["dkall"], b["dvall"] = z(Rk, L * ld, dt=ct), z(Rk, L * ld, dt=ct)
            b["dWf"] = [z(2 * d, d) for _ in range(L)]              # folded K/V weight gradients (per backward)
            b["dbf"] = self._acc0[self._acc_off: self._acc_off + L * 2 * d].view(L, 2 * d)   # folded K/V bias gradients
            self._acc_off += (L * 2 * d + 15) // 16 * 16
        # per-layer activations: shape(i) -- query-side tensors follow Rl / Tl, key / value-side ones stay full (qh .. lse:
        # the cross-attention block's, or the self-attention block's in a self-only plan, where S == T)
        acts = [("xn", lambda i: (R, ld), ct),
                ("qh", lambda i: (B, H, Tl[i], dhp), ct), ("kh", lambda i: (B, H, e.S, dhp), ct),
                ("vh", lambda i: (B, H, e.S, dhp), ct), ("ao", lambda i: (Rl[i], ld), ct),
                ("lse", lambda i: (B, H, Tl[i]), torch.float32),
                ("xmid", lambda i: (Rl[i], d), torch.float32), ("xn2", lambda i: (Rl[i], ld), ct),
                ("h1", lambda i: (Rl[i], ld4), ct),
                ("st0m", lambda i: (R,), torch.float32), ("st0r", lambda i: (R,), torch.float32),
                ("st1m", lambda i: (Rl[i],), torch.float32), ("st1r", lambda i: (Rl[i],), torch.float32)]
        if self._kv and c.biprojection:
            acts += [("qs", lambda i: (B, H, Tl[i], dhp), ct), ("ks", lambda i: (B, H, e.T, dhp), ct),
                     ("vs", lambda i: (B, H, e.T, dhp), ct), ("aos", lambda i: (Rl[i], ld), ct),
                     ("lses", lambda i: (B, H, Tl[i]), torch.float32), ("xmid0", lambda i: (Rl[i], d), torch.float32),
                     ("xq", lambda i: (Rl[i], ld), ct), ("st2m", lambda i: (Rl[i],), torch.float32),
                     ("st2r", lambda i: (Rl[i],), torch.float32)]
        for nm, shape, dt in acts:
            b[nm] = [z(*shape(i), dt=dt) for i in range(L)]
        if tailp:
            # last layer: rows {0, T-1} of its input (fp32) and of LN0(input) (CT), their gradients, and the residual
            # gradient scattered back into an otherwise-zero [R, d] buffer (only the two row blocks are ever written)
            b["xg"], b["xng"] = z(2 * B, d), z(2 * B, ld, dt=ct)
            b["dxg"], b["dxng"], b["dxs"] = z(2 * B, d), z(2 * B, d), z(R, d)
        # backward temporaries (shared by all layers)
        b["dx"], b["dxn"] = z(R, d), z(R, d)
        # Off-critical-path work (weight gradients, the key/value-side dgrad + LayerNorm backward) runs on a
        # side stream up to two layers behind the main chain, so every operand it reads has its own buffer
        # within a layer (dyf: FFN, dy: attention, dy0/dqs/dks/dvs: biprojection self-attention half) and is
        # double-buffered by layer parity.
        two = lambda *shape: [z(*shape, dt=ct), z(*shape, dt=ct)]
        b["dy"], b["dh1"] = two(R, ld), two(R, ld4)
        # dyf[i % 3]: written one layer early (fused into the LayerNorm backward that produces dx)
        b["dyf"] = [z(R, ld, dt=ct) for _ in range(3)]
        if self._kv:
            b["dq"] = two(R, ld)
        if self._kv and c.biprojection:
            b["dy0"] = two(R, ld)
        if has_self:
            # dQ | dK | dV of the self-attention block side by side in one [R, 3 ld] buffer: without column padding
            # (ld == d) that is the [R, 3d] operand of ONE d(xn) = [dq dk dv] in_proj_weight product (K = 3d) instead
            # of three K = d launches accumulating into the same output
            # (one spare row: the bounded loaders size their descriptors rows x ld from each VIEW's first element, so
            # the dK / dV views' ranges reach up to 2 ld elements past row R - 1)
            b["dqkvs"] = two(R + 1, 3 * ld)
            b["dqs"], b["dks"], b["dvs"] = ([t[:R, w * ld:(w + 1) * ld] for t in b["dqkvs"]] for w in range(3))
        if self._kv:
            # read by the side-stream dK/dV pass of the cross attention: by layer parity like dq/dk/dv
            b["dao"] = [z(B, H, e.T, dhp, dt=ct) for _ in range(2)]
            b["delta"] = [z(B, H, e.T) for _ in range(2)]
        if has_self:                                       # the self-attention backward runs on the main stream: one buffer
            k = _BIP_SELF_KEYS if self._kv else _SELF_KEYS
            b[k["dao"]], b[k["delta"]] = z(B, H, e.T, dhp, dt=ct), z(B, H, e.T)
        if self._kv:
            if not self._kv_fused:
                b["dke"], b["dve"] = z(Rk, d), z(Rk, d)
            b["dxk"], b["dxv"] = z(e.S, B, d), z(e.S, B, d)
        b["dxq"] = z(e.T, B, d)
        if self._masked:
            # key visibility of the plan's last forward, one byte per (sample, key), nonzero = visible: written by forward()
            # as bool (torch.eq's own output type, one launch), read by the kernels through the uint8 view of the same bytes
            for nm, n in ((("vis_s", e.T),) if has_self else ()) + ((("vis_c", e.S),) if self._kv else ()):
                b[nm + "_b"] = torch.ones(B, n, device=dev, dtype=torch.bool)
                b[nm] = b[nm + "_b"].view(torch.uint8)
        return b

    # -- helpers ----------------------------------------------------------------
    def _mask_off(self, T: int, S: int) -> int:
        return 1 + abs(S - T) if self.cfg.attn_mask else 0

    def _pn(self, e: EncoderDesc, i: int, leaf: str) -> str:
        return f"{e.prefix}layers.{i}.{leaf}"

    def _gemm(self, variant, probs, background=False, presplit=()):
        # every operand of the encoder GEMMs is a CT buffer written by this library (LayerNorm / cast / epilogue /
        # attention outputs into zero-initialised padded rows, packed weight shadows): the k padding is zero
        # background: weight gradients only.  The side stream's K/V projections and K/V dgrads measured better WITH the
        # critical-path issue priority (16.79 -> 16.73 ms/step): the forward ones gate the next attention
        for p in probs:
            p.flags |= F_KPAD | (F_BACKGROUND if background else 0)
        arr = ops.array(GemmProblem, probs)
        arr.x3 = self.x3                             # bf16x3 mode: ops.gemm_grouped splits the operands of eligible launches
        # ... except operands whose split image an earlier launch of the same step has left: the forward activations a
        # weight gradient reads again, and gradients the main stream's data-gradient product of this layer has just split
        arr.x3_presplit = frozenset(t.data_ptr() for t in presplit)
        return (ops.gemm_grouped, self.dtype, variant, arr)

    def _tail(self, b: dict, i: int) -> bool:
        """Layer i runs on rows {0, T-1} only (EncoderDesc.tail_rows, last layer)."""
        return b["tailp"] and i == self.cfg.layers - 1

    def _bias_route(self, gptr):
        """Where a linear layer's bias gradient (a device address) is summed: (on the epilogue / row kernel that has the
        fp32 values -- float atomics or the LayerNorm workspace, the default --, as colsum_a of the layer's weight-gradient
        product -- deterministic mode: one owner per column, k ascending, over the values as stored in CT).  One is None."""
        return (None, gptr) if self.det else (gptr, None)

    # -- per-block problem builders -------------------------------------------------
    # Each appends encoder e's problems of layer i to the layer's launch lists t[name] (one launch per name, problems in
    # encoder order).  The caller passes what differs between the layer kinds: inputs, residuals, first-writer flags, drop
    # sites, buffer keys.  pr(p): the dropout probability p in training, 0 in eval.
    def _proj(self, e, i, Ain, rows, which, Cout, Tlen):
        """Q (which 0, scaled), K (1) or V (2) projection of in_proj_weight into head-major Cout."""
        d, ld = self.cfg.d, self.ld
        return ops.gemm_problem(Ain, self.store.sptr(self._pn(e, i, "self_attn.in_proj_weight"), which * d * ld), Cout, rows, d, d,
                                ld, ld, 0, bias_n=self.store.p(self._pn(e, i, "self_attn.in_proj_bias"))[which * d:(which + 1) * d],
                                alpha=self.scale if which == 0 else 1.0, out_kind=OUT_HEADS,
                                heads=(self.B, self.cfg.H, Tlen, self.dh, self.dhp))

    def _ln0_fwd(self, t, e, b, i):
        P = lambda leaf: self.store.p(self._pn(e, i, leaf))
        t["ln0"].append(ops.ln_problem(b["x"][i], P("layer_norms.0.weight"), P("layer_norms.0.bias"), b["st0m"][i], b["st0r"][i],
                                       b["R"], out=b["xn"][i], ldo=self.ld))

    def _ln0_bwd(self, t, e, b, i, pr):
        """LayerNorm-0 backward over all rows from d(xn), added to the residual gradient (the gathered rows' one, scattered
        into dxs, in a tail_rows last layer) into the dense dx the layers below continue from.  Hand-off to the next layer
        down (i-1): its FFN-output gradient dyf = dropmask(dx) and fc2.bias gradient are fused into this launch."""
        st, c, d = self.store, self.cfg, self.cfg.d
        nxt = {} if i == 0 else dict(cast=b["dyf"][(i - 1) % 3], ldc=self.ld,
                                     cast_colsum=self._bias_route(st.gptr(self._pn(e, i - 1, "fc2.bias")))[0],
                                     drop_p=pr(c.res_dropout), drop_site=site(e.enc_id, i - 1, S_RES2))
        t["ln0"].append(ops.ln_problem(b["x"][i], st.p(self._pn(e, i, "layer_norms.0.weight")), None, b["st0m"][i], b["st0r"][i],
                                       b["R"], dy=b["dxn"], ldy=d, add=b["dxs"] if self._tail(b, i) else b["dx"], dx=b["dx"],
                                       dgamma=st.gptr(self._pn(e, i, "layer_norms.0.weight")),
                                       dbeta=st.gptr(self._pn(e, i, "layer_norms.0.bias")), **nxt))

    def _self_attn_fwd(self, t, e, b, i, pr, k, res_site):
        """Self-attention over LN0(x) (transformer.py:158-159): keys / values from every row, queries from the layer's
        query rows; b[k["mid"]] = x + drop(out_proj(attention)) (dropout site res_site).  LN0 is _ln0_fwd."""
        st, c, B, d, H, ld = self.store, self.cfg, self.B, self.cfg.d, self.cfg.H, self.ld
        R, Rq, Tq = b["R"], b["Rl"][i], b["Tl"][i]
        x_in, xn = b["x"][i], b["xn"][i]
        xq_in, res_in = xn, x_in                           # query operand, its residual
        tail = self._tail(b, i)
        if tail:
            # time steps 0 and T-1 are the first and the last B rows of a [T, B, .] tensor: two block copies
            for j, r0 in ((0, 0), (1, R - B)):
                t["s.gather"].append(ops.cast_problem(x_in[r0:r0 + B], d, B, d, dst_f32=b["xg"][j * B:(j + 1) * B], ldf=d))
                t["s.gather"].append(ops.cast_problem(xn[r0:r0 + B], ld, B, d, a_is_ct=True, dst_ct=b["xng"][j * B:(j + 1) * B],
                                                      ldd=ld))
            xq_in, res_in = b["xng"], b["xg"]
        q, kk, v, o, lse = (b[k[n]][i] for n in ("q", "k", "v", "o", "lse"))
        t["s.qkv"] += [self._proj(e, i, xq_in, Rq, 0, q, Tq), self._proj(e, i, xn, R, 1, kk, e.T), self._proj(e, i, xn, R, 2, v, e.T)]
        t["s.att"].append(ops.attn_problem(q, kk, v, o, ld, lse, B, H, Tq, e.T, self.dh, self.dhp, self._mask_off(e.T, e.T),
                                           drop_p=pr(e.attn_dropout), drop_site=site(e.enc_id, i, S_ATTN_SELF),
                                           **(dict(q_pos0=0, q_stride=e.T - 1) if tail else {})))
        t["s.out"].append(ops.gemm_problem(o, st.sptr(self._pn(e, i, "self_attn.out_proj.weight")), b[k["mid"]][i], Rq, d, d, ld, ld,
                                           d, bias_n=st.p(self._pn(e, i, "self_attn.out_proj.bias")), resid=res_in, ldr=d,
                                           drop_p=pr(c.res_dropout), drop_site=site(e.enc_id, i, res_site)))

    def _self_attn_bwd(self, t, e, b, i, pr, k, first, acc1, cast=None):
        """Backward of _self_attn_fwd down to d(xn) (dQ | dK | dV side by side in dqkvs); LN0 is _ln0_bwd.  first: flags of
        the out_proj.weight / in_proj_weight rows [0, d) gradients (accumulating when another block wrote them first);
        acc1: those of rows [d, 3d).  cast = (dx, res_site): d(out_proj output) is dropmask(dx), not the FFN's hand-off."""
        st, c, B, d, H, ld = self.store, self.cfg, self.B, self.cfg.d, self.cfg.H, self.ld
        R, Rq, Tq = b["R"], b["Rl"][i], b["Tl"][i]
        GP = lambda leaf, off=0: st.gptr(self._pn(e, i, leaf), off)
        ipw, wo = self._pn(e, i, "self_attn.in_proj_weight"), self._pn(e, i, "self_attn.out_proj.weight")
        par = i & 1
        dy, dqs, dks, dvs = b[k["dy"]][par], b["dqs"][par], b["dks"][par], b["dvs"][par]
        q, kk, v, o, lse, dao, delta = (b[k[n]] for n in ("q", "k", "v", "o", "lse", "dao", "delta"))
        q, kk, v, o, lse = q[i], kk[i], v[i], o[i], lse[i]
        tail = self._tail(b, i)
        xn = b["xn"][i]
        xq_in = b["xng"] if tail else xn
        ob_sum, ob_ride = self._bias_route(GP("self_attn.out_proj.bias"))
        if cast is not None:
            t["s.cast"].append(ops.cast_problem(cast[0], d, Rq, d, dst_ct=dy, ldd=ld, colsum=ob_sum,
                                                drop_p=pr(c.res_dropout), drop_site=site(e.enc_id, i, cast[1])))
        t["s.acts"] += [o, xq_in, xn]
        t["s.wg"].append(ops.gemm_problem(dy, o, GP("self_attn.out_proj.weight"), d, d, Rq, ld, ld, d, flags=first, colsum_a=ob_ride))
        t["s.dgout"].append(ops.gemm_problem(dy, st.sptr(wo), dao, Rq, d, d, ld, ld, 0, out_kind=OUT_HEADS,
                                             heads=(B, H, Tq, self.dh, self.dhp)))
        t["s.att"].append(ops.attn_problem(q, kk, v, o, ld, lse, B, H, Tq, e.T, self.dh, self.dhp, self._mask_off(e.T, e.T),
                                           dO=dao, delta=delta, dQ=dqs, lddq=3 * ld, dK=dks, lddk=3 * ld, dV=dvs, lddv=3 * ld,
                                           dq_scale=self.scale, drop_p=pr(e.attn_dropout), drop_site=site(e.enc_id, i, S_ATTN_SELF),
                                           **(dict(q_pos0=0, q_stride=e.T - 1) if tail else {})))
        # in_proj_weight row blocks [0, d), [d, 2d), [2d, 3d) (with a key / value source, unfold_grads comes after this
        # launch and adds to rows [d, 3d))
        for w, src, xin, rows in ((0, dqs, xq_in, Rq), (1, dks, xn, R), (2, dvs, xn, R)):
            t["s.wg"].append(ops.gemm_problem(src, xin, st.gptr(ipw, w * d * d), d, d, rows, 3 * ld, ld, d,
                                              flags=first if w == 0 else acc1,
                                              colsum_a=GP("self_attn.in_proj_bias", w * d)))
        # d(xn) = dq Wq + dk Wk + dv Wv: three launches (plain store, then two +=) -- one owner per
        # output tile in each launch, no atomics (per-lane-scattered float atomics run ~17x below store rate)
        if tail:
            # keys / values come from every row, the query only from rows {0, T-1}: d(xn) over all rows is the
            # K / V part; the query part is a [2B, d] product whose row blocks are added into it, and the
            # gathered rows' residual gradient goes to the same two row blocks of the otherwise-zero dxs
            if ld == d:
                t["s.dg_a"].append(ops.gemm_problem(b["dqkvs"][par][:R, ld:], st.sptr(ipw, d * ld), b["dxn"], R, d, 2 * d,
                                                    3 * ld, ld, d))
            else:
                t["s.dg_a"].append(ops.gemm_problem(dks, st.sptr(ipw, d * ld), b["dxn"], R, d, d, 3 * ld, ld, d))
                t["s.dg_b"].append(ops.gemm_problem(dvs, st.sptr(ipw, 2 * d * ld), b["dxn"], R, d, d, 3 * ld, ld, d, flags=F_ACCUM))
            t["s.dgq"].append(ops.gemm_problem(dqs, st.sptr(ipw, 0), b["dxng"], Rq, d, d, 3 * ld, ld, d))
            for j, r0 in ((0, 0), (1, R - B)):
                blk = slice(j * B, (j + 1) * B)
                t["s.scatter"].append(ops.addn_problem(b["dxn"][r0:r0 + B], [b["dxn"][r0:r0 + B], b["dxng"][blk]]))
                t["s.scatter"].append(ops.addn_problem(b["dxs"][r0:r0 + B], [b["dxg"][blk]]))
        elif ld == d:                                   # one product over K = 3d (see the dqkvs buffer)
            t["s.dg_a"].append(ops.gemm_problem(b["dqkvs"][par], st.sptr(ipw, 0), b["dxn"], R, d, 3 * d, 3 * ld, ld, d))
        else:
            t["s.dg_a"].append(ops.gemm_problem(dqs, st.sptr(ipw, 0), b["dxn"], R, d, d, 3 * ld, ld, d))
            t["s.dg_b"].append(ops.gemm_problem(dks, st.sptr(ipw, d * ld), b["dxn"], R, d, d, 3 * ld, ld, d, flags=F_ACCUM))
            t["s.dg_c"].append(ops.gemm_problem(dvs, st.sptr(ipw, 2 * d * ld), b["dxn"], R, d, d, 3 * ld, ld, d, flags=F_ACCUM))

    def _cross_attn_fwd(self, t, e, b, i, pr, q_src, resid):
        """Cross attention: queries projected from q_src (CT), keys / values from the normalised key / value source through
        the LayerNorm-folded K / V weights (on the side stream, t["c.kv"]); xmid = resid + drop(out_proj(attention))."""
        st, c, B, d, H, ld = self.store, self.cfg, self.B, self.cfg.d, self.cfg.H, self.ld
        Rq, Tq = b["Rl"][i], b["Tl"][i]
        qpos = dict(q_pos0=0, q_stride=e.T - 1) if self._tail(b, i) else dict(q_pos0=e.q_pos0, q_stride=e.q_stride)
        kvf = self._pn(e, i, KVF)
        t["c.q"].append(self._proj(e, i, q_src, Rq, 0, b["qh"][i], Tq))
        for w, hat, dst in ((0, b["khat"], b["kh"][i]), (1, b["vhat"], b["vh"][i])):    # folded: khat (W_k * gamma)^T + (W_k beta + b_k)
            t["c.kv"].append(ops.gemm_problem(hat, st.sptr(kvf + (".v" if w else ".k")), dst, b["Rk"], d, d, ld, ld, 0,
                                              bias_n=st.fold(kvf, w * d, d), out_kind=OUT_HEADS, heads=(B, H, e.S, self.dh, self.dhp)))
        t["c.att"].append(ops.attn_problem(b["qh"][i], b["kh"][i], b["vh"][i], b["ao"][i], ld, b["lse"][i], B, H, Tq, e.S, self.dh,
                                           self.dhp, self._mask_off(e.T_full or e.T, e.S), drop_p=pr(e.attn_dropout),
                                           drop_site=site(e.enc_id, i, S_ATTN), **qpos))
        t["c.out"].append(ops.gemm_problem(b["ao"][i], st.sptr(self._pn(e, i, "self_attn.out_proj.weight")), b["xmid"][i], Rq, d, d,
                                           ld, ld, d, bias_n=st.p(self._pn(e, i, "self_attn.out_proj.bias")), resid=resid, ldr=d,
                                           drop_p=pr(c.res_dropout), drop_site=site(e.enc_id, i, S_RES1)))

    def _cross_attn_bwd(self, t, e, b, i, pr, acc1, q_src, dq_out, dq_flags):
        """Backward of _cross_attn_fwd: d(query operand) into dq_out (dq_flags), the key side as dK / dV blocks of dkall /
        dvall or low-rank (_lowrank), the folded K / V gradients into dWf / dbf (unfolded per layer by unfold_grads)."""
        st, c, B, d, H, ld = self.store, self.cfg, self.B, self.cfg.d, self.cfg.H, self.ld
        Rq, Tq, Rk = b["Rl"][i], b["Tl"][i], b["Rk"]
        qpos = dict(q_pos0=0, q_stride=e.T - 1) if self._tail(b, i) else dict(q_pos0=e.q_pos0, q_stride=e.q_stride)
        GP = lambda leaf, off=0: st.gptr(self._pn(e, i, leaf), off)
        ipw = self._pn(e, i, "self_attn.in_proj_weight")
        lr = self._lowrank
        par = i & 1
        dy, dq, dao, delta = (b[n][par] for n in ("dy", "dq", "dao", "delta"))
        ldk = c.layers * ld                       # layer i's dK / dV: column block i of dkall / dvall
        dk, dv = (None, None) if lr else (b["dkall"][:, i * ld:(i + 1) * ld], b["dvall"][:, i * ld:(i + 1) * ld])
        t["c.grads"] += [dy, dq]
        t["c.acts"] += [b["ao"][i], q_src] + ([] if lr else [b["khat"], b["vhat"]])
        # (the first writer of out_proj.weight / in_proj_weight rows [0, d) on the side stream; a biprojection
        # self-attention block below comes second and accumulates)
        t["c.wg"].append(ops.gemm_problem(dy, b["ao"][i], GP("self_attn.out_proj.weight"), d, d, Rq, ld, ld, d, flags=acc1,
                                          colsum_a=self._bias_route(GP("self_attn.out_proj.bias"))[1]))
        t["c.dgout"].append(ops.gemm_problem(dy, st.sptr(self._pn(e, i, "self_attn.out_proj.weight")), dao, Rq, d, d, ld, ld, 0,
                                             out_kind=OUT_HEADS, heads=(B, H, Tq, self.dh, self.dhp)))
        lrx = {}
        if lr:
            HT, Sp = H * Tq, b["Sp"]
            rows = HT * B                        # row (h*T + t)*B + b everywhere below
            lrx = dict(dS=b["dSall"][i], Pd=b["Pdall"][i], xs=(Sp, Tq * B * Sp, B * Sp))
        t["c.att"].append(ops.attn_problem(b["qh"][i], b["kh"][i], b["vh"][i], b["ao"][i], ld, b["lse"][i], B, H, Tq, e.S, self.dh,
                                           self.dhp, self._mask_off(e.T_full or e.T, e.S), dO=dao, delta=delta, dQ=dq, lddq=ld,
                                           dK=dk, lddk=ldk, dV=dv, lddv=ldk, dq_scale=self.scale,
                                           drop_p=pr(e.attn_dropout), drop_site=site(e.enc_id, i, S_ATTN), **qpos, **lrx))
        # query projection: gradients go straight to the parameters.  Key / value projections ran with the
        # LayerNorm folded in: their bias column sums and weight gradients (against khat / vhat) land in
        # per-layer scratch and are unfolded into in_proj / LayerNorm gradients by one launch at the end.
        # (the bias column sums ride on the weight-gradient GEMMs: colsum_a, one extra MFMA against ones)
        t["c.wg"].append(ops.gemm_problem(dq, q_src, st.gptr(ipw, 0), d, d, Rq, ld, ld, d, flags=acc1,
                                          colsum_a=GP("self_attn.in_proj_bias")))
        if lr:
            qexp, doexp, U, Av = (b[n][par] for n in ("qexp", "doexp", "U", "Av"))
            # heads' q / dO vectors as block rows; the folded value-bias gradient = sum rowsum(Pd) dO (the folded key
            # bias gets none: the rows of dS sum to zero -- dbf's key half stays at the zero every backward starts from)
            t["c.expand"].append(ops.expand_problem(b["qh"][i], dao, qexp, doexp, B, H, Tq, self.dh, self.dhp, ld, Pd=b["Pdall"][i],
                                                    S=Sp, dbias=b["dbf"][i][d:]))
            for src, stack, dst in ((qexp, KSTACK, b["qkall"][i]), (doexp, VSTACK, b["daall"][i])):
                t["c.lrqk"].append(ops.gemm_problem(src, st.sptr(e.prefix + stack, i * ld * ld), dst, rows, d, d, ld, ld, ld,
                                                    out_kind=OUT_CT))
            # per batch element: [H T, S] x [S, d]; the rows of a batch element are B rows apart in all three tensors
            for mat, hat_, dst in ((b["dSall"][i], b["khat"], U), (b["Pdall"][i], b["vhat"], Av)):
                t["c.lrqk"].append(ops.gemm_problem(mat, hat_, dst, HT, d, e.S, B * Sp, B * ld, B * ld, out_kind=OUT_CT,
                                                    flags=F_CT_NARROW, batch=(B, Sp, ld, ld)))
            t["c.wg"].append(ops.gemm_problem(qexp, U, b["dWf"][i][:d], d, d, rows, ld, ld, d))
            t["c.wg"].append(ops.gemm_problem(doexp, Av, b["dWf"][i][d:], d, d, rows, ld, ld, d))
        else:
            t["c.wg"].append(ops.gemm_problem(dk, b["khat"], b["dWf"][i][:d], d, d, Rk, ldk, ld, d, colsum_a=b["dbf"][i][:d]))
            t["c.wg"].append(ops.gemm_problem(dv, b["vhat"], b["dWf"][i][d:], d, d, Rk, ldk, ld, d, colsum_a=b["dbf"][i][d:]))
        t["c.dgq"].append(ops.gemm_problem(dq, st.sptr(ipw, 0), dq_out, Rq, d, d, ld, ld, d, flags=dq_flags))

    def _ffn_fwd(self, t, e, b, i, pr, stats):
        """x[i+1] = xmid + drop(fc2(drop(relu(fc1(LN_F xmid))))); stats: LN_F's mean / rstd buffers."""
        st, c, d, ld, ld4 = self.store, self.cfg, self.cfg.d, self.ld, self.ld4
        P = lambda leaf: st.p(self._pn(e, i, leaf))
        Rq = b["Rl"][i]
        t["f.ln"].append(ops.ln_problem(b["xmid"][i], P(f"layer_norms.{self._lnF}.weight"), P(f"layer_norms.{self._lnF}.bias"),
                                        stats[0], stats[1], Rq, out=b["xn2"][i], ldo=ld))
        t["f.fc1"].append(ops.gemm_problem(b["xn2"][i], st.sptr(self._pn(e, i, "fc1.weight")), b["h1"][i], Rq, 4 * d, d, ld, ld, ld4,
                                           bias_n=P("fc1.bias"), flags=F_RELU, drop_p=pr(c.relu_dropout),
                                           drop_site=site(e.enc_id, i, S_RELU), out_kind=OUT_CT))
        t["f.fc2"].append(ops.gemm_problem(b["h1"][i], st.sptr(self._pn(e, i, "fc2.weight")), b["x"][i + 1], Rq, d, 4 * d, ld4, ld4, d,
                                           bias_n=P("fc2.bias"), resid=b["xmid"][i], ldr=d, drop_p=pr(c.res_dropout),
                                           drop_site=site(e.enc_id, i, S_RES2)))

    def _ffn_bwd(self, t, e, b, i, pr, acc1, dx, stats):
        """Backward of _ffn_fwd from dyf (written by the layer above) down to xmid; the LN_F backward adds into the residual
        gradient dx and hands d(out_proj output) = dropmask(dx) (site S_RES1) to the attention block below as dy."""
        st, c, d, ld, ld4 = self.store, self.cfg, self.cfg.d, self.ld, self.ld4
        GP = lambda leaf: st.gptr(self._pn(e, i, leaf))
        Rq = b["Rl"][i]
        dh1, dy, dyf = b["dh1"][i & 1], b["dy"][i & 1], b["dyf"][i % 3]
        inv_relu = 1.0 / (1.0 - pr(c.relu_dropout))
        t["f.grads"] += [dyf, dh1]
        t["f.acts"] += [b["h1"][i], b["xn2"][i]]
        b1_sum, b1_ride = self._bias_route(GP("fc1.bias"))
        t["f.wg"].append(ops.gemm_problem(dyf, b["h1"][i], GP("fc2.weight"), d, 4 * d, Rq, ld, ld4, 4 * d, flags=acc1,
                                          colsum_a=self._bias_route(GP("fc2.bias"))[1]))
        t["f.dg2"].append(ops.gemm_problem(dyf, st.sptr(self._pn(e, i, "fc2.weight")), dh1, Rq, 4 * d, d, ld, ld4, ld4,
                                           gate=b["h1"][i], ldg=ld4, gate_scale=inv_relu, colsum=b1_sum, out_kind=OUT_CT))
        t["f.wg"].append(ops.gemm_problem(dh1, b["xn2"][i], GP("fc1.weight"), 4 * d, d, Rq, ld4, ld, d, flags=acc1, colsum_a=b1_ride))
        t["f.dg1"].append(ops.gemm_problem(dh1, st.sptr(self._pn(e, i, "fc1.weight")), b["dxn"], Rq, d, 4 * d, ld4, ld, d))
        lnF = self._lnF
        t["f.ln"].append(ops.ln_problem(b["xmid"][i], st.p(self._pn(e, i, f"layer_norms.{lnF}.weight")), None, stats[0], stats[1], Rq,
                                        dy=b["dxn"], ldy=d, add=dx, dx=dx, dgamma=GP(f"layer_norms.{lnF}.weight"),
                                        dbeta=GP(f"layer_norms.{lnF}.bias"), cast=dy, ldc=ld,
                                        cast_colsum=self._bias_route(GP("self_attn.out_proj.bias"))[0], drop_p=pr(c.res_dropout),
                                        drop_site=site(e.enc_id, i, S_RES1)))

    # -- forward tables ---------------------------------------------------------
    def _build_fwd(self, training: bool):
        c, st, d, A = self.cfg, self.store, self.cfg.d, ops.array
        pr = (lambda p: p) if training else (lambda p: 0.0)
        ln = lambda probs: (ops.ln_fwd, self.dtype, A(LnProblem, probs), d)
        nt = lambda probs: self._gemm(GEMM_NT, probs)
        # km: the block's key masks in a masked plan (_km_self / _km_cross), one per problem: the same step, the *_kmask entry
        attn = lambda probs, km: (ops.attn_fwd, self.dtype, A(AttnProblem, probs)) if km is None else \
            (ops.attn_fwd_kmask, self.dtype, A(AttnProblem, probs), km)
        steps, kv_steps = [], []
        if self._kv_fused:
            kv_steps = [(SIDE, (ops.kv_source_fwd, self.dtype, self._kvsrc[training], self.table, d, math.sqrt(d))), (MARK, "hat")]
        elif self._kv:
            hat = []
            for b in self.buf:
                hat += [ops.ln_problem(b["ke"], self._ones, self._zeros, b["stk"][0], b["stk"][1], b["Rk"], out=b["khat"], ldo=self.ld),
                        ops.ln_problem(b["ve"], self._ones, self._zeros, b["stv"][0], b["stv"][1], b["Rk"], out=b["vhat"], ldo=self.ld)]
            kv_steps = [(SIDE, ln(hat)), (MARK, "hat")]
        for i in range(c.layers):
            t = defaultdict(list)
            for e, b in zip(self.encs, self.buf):
                self._ln0_fwd(t, e, b, i)
                if not self._kv:                           # self-only: self + FFN
                    self._self_attn_fwd(t, e, b, i, pr, _SELF_KEYS, S_RES1)
                    self._ffn_fwd(t, e, b, i, pr, (b["st1m"][i], b["st1r"][i]))
                elif c.biprojection:                       # self + cross (queries: the self block's output, not normalised) + FFN
                    self._self_attn_fwd(t, e, b, i, pr, _BIP_SELF_KEYS, S_RES0)
                    t["s.cast"].append(ops.cast_problem(b["xmid0"][i], d, b["Rl"][i], d, dst_ct=b["xq"][i], ldd=self.ld))
                    self._cross_attn_fwd(t, e, b, i, pr, b["xq"][i], b["xmid0"][i])
                    self._ffn_fwd(t, e, b, i, pr, (b["st2m"][i], b["st2r"][i]))
                else:                                      # crossmodal: cross (queries: LN0(x)) + FFN
                    self._cross_attn_fwd(t, e, b, i, pr, b["xn"][i], b["x"][i])
                    self._ffn_fwd(t, e, b, i, pr, (b["st1m"][i], b["st1r"][i]))
            self_half = lambda: [ln(t["ln0"])] + ([(ops.rows_cast, self.dtype, A(CastProblem, t["s.gather"]))] if t["s.gather"] else []) \
                + [nt(t["s.qkv"]), attn(t["s.att"], self._km_self), nt(t["s.out"])]
            # K/V side of every layer depends only on the (embedded) key/value sources: the side stream runs it
            # ahead of the query chain; the main stream waits for layer i's K/V heads just before attention i.
            cross = lambda: [nt(t["c.q"]), (WAIT, i), attn(t["c.att"], self._km_cross), nt(t["c.out"])]
            ffn = [ln(t["f.ln"]), nt(t["f.fc1"]), nt(t["f.fc2"])]
            if not self._kv:
                steps += self_half() + ffn
            elif c.biprojection:
                steps += self_half() + [(ops.rows_cast, self.dtype, A(CastProblem, t["s.cast"]))] + cross() + ffn
            else:
                steps += [ln(t["ln0"])] + cross() + ffn
            if self._kv:
                kv_steps += [(SIDE, nt(t["c.kv"])), (MARK, i)]
        fin = [ops.ln_problem(b["x"][c.layers], st.p(e.prefix + "layer_norm.weight"), st.p(e.prefix + "layer_norm.bias"),
                              b["stf"][0], b["stf"][1], b["Rl"][-1], out=b["out"], ldo=d, out_f32=True)
               for e, b in zip(self.encs, self.buf)]
        steps.append(ln(fin))
        return kv_steps + steps + ([JOIN] if self._kv else [])


    @staticmethod
    def _exec(s, seed: int) -> None:
        """Run one step (fn, *args): every ops launch function takes its dropout seed as the keyword `seed`."""
        fn, *args = s
        if fn in ops.SEEDED:
            fn(*args, seed=seed)
        else:
            fn(*args)

    @staticmethod
    def _check_steps(steps) -> None:
        """Refuse, when the tables are built, a step whose function is not an ops launch function."""
        for s in steps:
            if s is JOIN or s[0] in (MARK, WAIT):
                continue
            fn = s[1][0] if s[0] in (SIDE, SIDE2) else s[0]
            if fn not in ops.STEP_FUNCTIONS:
                raise ValueError(f"launch table: {getattr(fn, '__name__', fn)!r} is not a step function (ops.STEP_FUNCTIONS)")

    def _run(self, steps, seed: int, on_mark=None) -> None:
        """Launch a step table.  Plain steps go to the current ("main") stream.  (SIDE, step) goes to the side
        stream, ordered behind everything the main stream has launched so far; (MARK, k) records an event on the
        side stream; (WAIT, k) makes the main stream wait for mark k (no-op if it was never recorded); JOIN
        makes the main stream wait for all side work.  With BPMULT_SIDE=0 everything runs on the main stream."""
        if not _SIDE:
            for s in steps:
                if s is not JOIN and s[0] is MARK and on_mark is not None:
                    ev = torch.cuda.Event()
                    ev.record(torch.cuda.current_stream())
                    on_mark(s[1], [ev])
                if s is JOIN or s[0] is MARK or s[0] is WAIT:
                    continue
                self._exec(s[1] if s[0] in (SIDE, SIDE2) else s, seed)
            return
        main = torch.cuda.current_stream()
        side = _side_stream(main.device, 1, self._side_low)
        marks: Dict[int, torch.cuda.Event] = {}
        main_dirty, side_dirty = True, False
        for s in steps:
            if s is JOIN:
                if side_dirty:
                    ev = torch.cuda.Event()
                    ev.record(side)
                    main.wait_event(ev)
                    side_dirty = False
                    _OPEN_FORKS.pop(side.cuda_stream, None)
            elif s[0] is SIDE2:                     # third stream: starts right behind the main stream's last launch
                side2 = _side_stream(main.device, 2, self._side_low)
                ev = torch.cuda.Event()
                ev.record(main)
                side2.wait_event(ev)
                _OPEN_FORKS[side2.cuda_stream] = side2
                with torch.cuda.stream(side2):
                    self._exec(s[1], seed)
                ev2 = torch.cuda.Event()
                ev2.record(side2)
                side.wait_event(ev2)                # the side stream's later steps consume its output: joined through it
                _OPEN_FORKS.pop(side2.cuda_stream, None)
                _OPEN_FORKS[side.cuda_stream] = side
                side_dirty = True
            elif s[0] is SIDE:
                if main_dirty:
                    ev = torch.cuda.Event()
                    ev.record(main)
                    side.wait_event(ev)
                    main_dirty = False
                _OPEN_FORKS[side.cuda_stream] = side
                with torch.cuda.stream(side):
                    self._exec(s[1], seed)
                side_dirty = True
            elif s[0] is MARK:
                if side_dirty:
                    marks[s[1]] = torch.cuda.Event()
                    marks[s[1]].record(side)
                if on_mark is not None:             # everything launched for this mark so far, on both streams
                    evm = torch.cuda.Event()
                    evm.record(main)
                    on_mark(s[1], [evm] + ([marks[s[1]]] if s[1] in marks else []))
            elif s[0] is WAIT:
                if s[1] in marks:
                    main.wait_event(marks.pop(s[1]))
            else:
                self._exec(s, seed)
                main_dirty = True

    def forward(self, xq: Sequence[torch.Tensor], xk: Sequence[torch.Tensor], xv: Sequence[torch.Tensor], seed: int,
                training: bool, self_masks: Optional[Sequence[Optional[torch.Tensor]]] = None,
                cross_masks: Optional[Sequence[Optional[torch.Tensor]]] = None) -> List[torch.Tensor]:
        """xq[e]: fp32 [T_e,B,d]; xk[e], xv[e]: fp32 [S_e,B,d] key / value sources (the same tensor at every
        reference call site, mmtr.py:779-791; they still get independent embedding dropout, transformer.py:73-79).
        With fused key / value sources (the default) the plan keeps references to xk / xv until its next forward and
        backward() reads them again: like any tensor saved for a backward pass they must not be modified in between.
        self_masks[e] / cross_masks[e] (a masked plan: exactly the masks its EncoderMasks declare, None for the others):
        bool / uint8 [B, T_e] / [B, S_e] on the plan's device, any strides, nonzero = PADDING; each is turned into the
        plan's visibility buffer by one launch on the current stream, ahead of the tables -- no host synchronisation.  The
        buffers belong to the plan like its activations: backward() and attention_maps() read what the last forward left."""
        c, B, d = self.cfg, self.B, self.cfg.d
        p = c.embed_dropout if training else 0.0
        emb = []
        fills = []
        for what, given, nm in (("self", self_masks, "vis_s"), ("cross", cross_masks, "vis_c")):
            given = [None] * len(self.encs) if given is None else list(given)
            for e, b, m, t in zip(self.encs, self.buf, self.masks, given):
                want = m.self_keys if what == "self" else m.cross_keys
                if (t is not None) != want:
                    raise ValueError(f"encoder {e.prefix}: this plan was built {'with' if want else 'without'} a {what}-attention "
                                     f"key mask, the call comes {'without' if want else 'with'} one")
                if t is not None:
                    n = e.T if what == "self" else e.S
                    if t.dtype not in (torch.bool, torch.uint8) or tuple(t.shape) != (B, n):
                        raise ValueError(f"encoder {e.prefix}: {what}-attention key mask must be bool / uint8 [{B},{n}], got "
                                         f"{tuple(t.shape)} {t.dtype}")
                    fills.append((t, b[nm + "_b"]))
        if not self._kv:                        # one input per encoder (xk / xv are ignored and may be None)
            xk = xv = [None] * len(self.encs)
        for e, b, q, k, v in zip(self.encs, self.buf, xq, xk, xv):
            for t, n in ((q, e.T), (k, e.S), (v, e.S))[:3 if self._kv else 1]:
                if tuple(t.shape) != (n, B, d) or not t.is_contiguous() or t.dtype != torch.float32:
                    raise ValueError(f"encoder {e.prefix}: expected contiguous fp32 [{n},{B},{d}], got {tuple(t.shape)} {t.dtype}")
            emb.append(ops.embed_problem(q, b["x"][0], e.T, B, drop_p=p, drop_site=site(e.enc_id, 0, S_EMB_Q), pos0=e.q_pos0,
                                         pos_stride=e.q_stride))
            if self._kv and not self._kv_fused:
                emb += [ops.embed_problem(k, b["ke"], e.S, B, drop_p=p, drop_site=site(e.enc_id, 0, S_EMB_K)),
                        ops.embed_problem(v, b["ve"], e.S, B, drop_p=p, drop_site=site(e.enc_id, 0, S_EMB_V))]
        if self._kv_fused:
            # 16-byte accesses: a source that starts off such a boundary (a view into a larger tensor) is copied first
            al = lambda t: t if t.data_ptr() % 16 == 0 else t.clone()
            ks = [al(k) for k in xk]
            vs = [kk if v is k else al(v) for k, kk, v in zip(xk, ks, xv)]
            self._kv_keep = (ks, vs)
            for arr in self._kvsrc.values():
                for i, (k, v) in enumerate(zip(ks, vs)):
                    ops.set_kv_source(arr[i], k, v)
        self._maps_ok = False
        for t, vis in fills:                    # visible = (padding == 0): the one launch per mask
            torch.eq(t, 0, out=vis)
        ops.embed_pos_fwd(emb, self.table, d, math.sqrt(d), seed)
        self._last = (seed, training)
        self._run(self._fwd[training], seed)
        self._maps_ok = True
        return [b["out"] for b in self.buf]

    # -- attention maps -----------------------------------------------------------
    def _map_blocks(self, e: EncoderDesc, b: dict, i: int):
        """(block name, Q, K, lse, S, mask_off, q_pos0, q_stride, query_steps) of layer i's attention blocks, in the order
        the layer runs them: the operands and the visibility rule of the forward problem (_self_attn_fwd / _cross_attn_fwd)."""
        Tq = b["Tl"][i]
        tail = self._tail(b, i)
        if tail:
            qpos, steps = (0, e.T - 1), (0, e.T - 1)
        else:
            qpos = (e.q_pos0, e.q_stride)
            steps = None if e.T_full is None else tuple(e.q_pos0 + r * e.q_stride for r in range(Tq))
        out = []
        if self.cfg.biprojection or not self._kv:
            k = _BIP_SELF_KEYS if self._kv else _SELF_KEYS
            out.append(("self", b[k["q"]][i], b[k["k"]][i], b[k["lse"]][i], e.T, self._mask_off(e.T, e.T),
                        *((0, e.T - 1) if tail else (0, 1)), steps))
        if self._kv:
            out.append(("cross", b["qh"][i], b["kh"][i], b["lse"][i], e.S, self._mask_off(e.T_full or e.T, e.S), *qpos, steps))
        return out

    def maps_ready(self) -> None:
        """A captured graph of this plan's forward has just been replayed (no Python of forward() ran)."""
        self._maps_ok = True

    def attention_maps(self, encoders=None, layers=None, per_head: bool = False) -> List[List[Dict[str, AttentionMap]]]:
        """Head-averaged attention maps of the LAST forward of this plan: for each selected encoder (index or parameter
        prefix; None = all, in plan order) a list over the selected layers (None = all) of {block: AttentionMap}, block
        "cross" (crossmodal), "self" (self-only) or both (biprojection with a key / value source; self [B, Tq, T], cross
        [B, Tq, S]).  W[b, i, j] = (1/H) sum_h softmax(scores)[b, h, i, j]: the probabilities BEFORE attention dropout --
        the reference's second MultiheadAttention return value in eval mode and whenever attn_dropout == 0 -- and exactly 0
        where the mask hides key j.  Detached fp32 tensors, freshly allocated, contiguous [B, Tq, S].

        Nothing is kept for this by the forward: the maps are recomputed from the layer's Q / K / LSE buffers (bpm_attn_maps),
        in launches of up to BPM_MAX_GROUP problems on the current stream -- the stream the forward ran on, which its last
        step (JOIN) has made wait for the side stream's key / value projections.  Every backward builder only READS these
        three buffers (_self_attn_bwd / _cross_attn_bwd pass them as Q / K / lse inputs of the attention problems; the
        low-rank route also reads qh in bpm_expand_heads; gradients go to dq / dqkvs / dao / delta / dkall / dSall ...),
        for every layer kind, so maps may be taken before or after backward(), until the plan's next forward.  Before any
        forward, or after one that did not finish launching, this raises RuntimeError.

        per_head=True: the probabilities of every head instead of their mean (bpm_attn_head_maps), W[b, h, i, j], contiguous
        [B, H, Tq, S]; everything else as above (same buffers, same key masks, same query_steps, same rules about when).
        A per-head map is H times the averaged one: B * H * Tq * S * 4 bytes, about 100 MB at the headline shape (T = S =
        512), several GB for all maps of a model -- select `encoders` and `layers`."""
        if not self._maps_ok:
            raise RuntimeError("attention_maps: no finished forward pass of this plan (its Q / K / LSE buffers hold nothing to "
                               "compute the maps from); run forward first")
        L = self.cfg.layers
        if encoders is None:
            eidx = list(range(len(self.encs)))
        else:
            eidx = []
            for n in encoders:
                if isinstance(n, str):
                    pf = [k for k, e in enumerate(self.encs) if e.prefix in (n, n + ".")]
                    if not pf:
                        raise ValueError(f"attention_maps: no encoder {n!r} in this plan ({[e.prefix for e in self.encs]})")
                    eidx.append(pf[0])
                else:
                    if not 0 <= n < len(self.encs):
                        raise IndexError(f"attention_maps: encoder index {n} out of range ({len(self.encs)} encoders)")
                    eidx.append(n)
        lidx = list(range(L)) if layers is None else list(layers)
        for i in lidx:
            if not isinstance(i, int) or not 0 <= i < L:
                raise IndexError(f"attention_maps: layer {i!r} out of range ({L} layers)")
        dev = self.store.device
        probs, res = [], []
        kms = []                                 # masked plan: each map's key mask, the visibility buffer its block's forward read
        for k in eidx:
            e, b = self.encs[k], self.buf[k]
            per_layer = []
            for i in lidx:
                maps = {}
                for name, q, kk, lse, S, moff, p0, st_, steps in self._map_blocks(e, b, i):
                    Tq = b["Tl"][i]
                    W = torch.empty((self.B, self.cfg.H, Tq, S) if per_head else (self.B, Tq, S), device=dev, dtype=torch.float32)
                    problem = ops.attn_head_map_problem if per_head else ops.attn_map_problem
                    probs.append(problem(q, kk, lse, W, S, self.B, self.cfg.H, Tq, S, self.dh, self.dhp, moff, q_pos0=p0, q_stride=st_))
                    if self._masked:
                        kms.append((b["vis_s" if name == "self" else "vis_c"], S))
                    maps[name] = AttentionMap(W, steps)
                per_layer.append(maps)
            res.append(per_layer)
        if probs and self._masked:
            (ops.attn_head_maps_kmask if per_head else ops.attn_maps_kmask)(self.dtype, probs, ops.attn_kmasks(kms))
        elif probs:
            (ops.attn_head_maps if per_head else ops.attn_maps)(self.dtype, probs)
        return res

    # -- backward tables --------------------------------------------------------
    def _build_bwd(self, training: bool, stores: bool = False):
        c, st, d, A = self.cfg, self.store, self.cfg.d, ops.array
        ACC1 = 0 if stores else F_ACCUM          # flags of the FIRST writer of a large weight gradient in a step
        pr = (lambda p: p) if training else (lambda p: 0.0)
        nn = lambda probs: self._gemm(GEMM_NN, probs)
        wg = lambda probs, presplit: (SIDE, self._gemm(GEMM_TN, probs, background=True, presplit=presplit))
        ln = lambda probs: (ops.ln_bwd, ops.ln_det(A(LnProblem, probs)) if self.det else A(LnProblem, probs), d, self.dtype)
        x3, lr = st.x3, self._lowrank
        steps = []
        for i in reversed(range(c.layers)):
            t = defaultdict(list)
            for e, b in zip(self.encs, self.buf):
                # residual-stream gradient of this layer's query rows: the two gathered rows in a tail_rows last layer
                # (its LayerNorm-0 backward over all rows then writes the dense dx the layers below continue from)
                dx = b["dxg"] if self._tail(b, i) else b["dx"]
                if not self._kv:                           # self-only: self + FFN, every block the first writer
                    self._ffn_bwd(t, e, b, i, pr, ACC1, dx, (b["st1m"][i], b["st1r"][i]))
                    self._self_attn_bwd(t, e, b, i, pr, _SELF_KEYS, ACC1, ACC1)
                elif c.biprojection:
                    # query was not normalised: its gradient joins the residual stream directly; the self-attention block
                    # comes second on out_proj.weight / in_proj_weight rows [0, d) and accumulates
                    self._ffn_bwd(t, e, b, i, pr, ACC1, dx, (b["st2m"][i], b["st2r"][i]))
                    self._cross_attn_bwd(t, e, b, i, pr, ACC1, b["xq"][i], dx, F_ACCUM)
                    self._self_attn_bwd(t, e, b, i, pr, _BIP_SELF_KEYS, F_ACCUM, ACC1, cast=(dx, S_RES0))
                else:
                    self._ffn_bwd(t, e, b, i, pr, ACC1, dx, (b["st1m"][i], b["st1r"][i]))
                    self._cross_attn_bwd(t, e, b, i, pr, ACC1, b["xn"][i], b["dxn"], 0)
                self._ln0_bwd(t, e, b, i, pr)
            for group in (t["f.ln"], t["ln0"]):              # each LayerNorm-backward launch owns its gradient rows exactly once
                ops.check_ln_rows(group, d)

            def ffn(presplit, wg_late):
                w = wg(t["f.wg"], presplit)
                return [nn(t["f.dg2"])] + ([] if wg_late else [w]) + [nn(t["f.dg1"])] + ([w] if wg_late else []) + [ln(t["f.ln"])]

            def self_half(presplit):
                # masked plan: bpm_attn_bwd's two passes (dQ + delta, then dK / dV) through their *_kmask entries, in its order
                satt = [(ops.attn_bwd, self.dtype, A(AttnProblem, t["s.att"]))] if self._km_self is None else \
                    [(ops.attn_bwd_dq_kmask, self.dtype, A(AttnProblem, t["s.att"]), self._km_self),
                     (ops.attn_bwd_dkv_kmask, self.dtype, A(AttnProblem, t["s.att"]), self._km_self)]
                return [nn(t["s.dgout"])] + satt + [wg(t["s.wg"], presplit),
                        nn(t["s.dg_a"])] + ([nn(t["s.dg_b"])] if t["s.dg_b"] else []) + ([nn(t["s.dg_c"])] if t["s.dg_c"] else []) + \
                    ([nn(t["s.dgq"]), (ops.add_n, A(AddnProblem, t["s.scatter"]))] if t["s.dgq"] else []) + [ln(t["ln0"])]

            if not self._kv:
                # Main stream: the data-gradient chain, the attention backward (dK / dV feed the d(xn) product on the
                # critical path, so both passes run here) and the LayerNorm backwards.  Side stream: the weight gradients.
                # bf16x3: only forward activations are listed as already split (their image is this step's forward
                # launch's); gradients are split again by the weight-gradient launch that reads them
                steps += [(WAIT, i + 2)] + ffn(t["f.acts"] if x3 else (), False) + self_half(t["s.acts"] if x3 else ()) + [(MARK, i)]
                continue
            # Ownership of parameter-gradient words (bpm_ln_bwd_ws adds its row sums with a plain read-modify-write):
            # layer_norms.* / out_proj.bias / fc2.bias gradients are written by the MAIN stream's LayerNorm backward
            # launches only, except layer_norms.{lnK} which unfold_grads (side stream) also adds to -- that launch is
            # ordered behind the LayerNorm-0 backward of layer i by the main_dirty event recorded before every SIDE step,
            # and the next main-stream writer of the same words is the NEXT step's backward (behind the JOIN).  Keep it
            # that way.
            # Side stream (SIDE): weight gradients and the key/value-side dgrad + LayerNorm backward -- nothing on
            # the backward critical path consumes them.  Temporaries are double-buffered by layer parity, so the
            # main chain only waits (WAIT) for the side work of two layers ago before overwriting them.
            wg_att = wg(t["c.wg"], t["c.grads"] + t["c.acts"] if x3 else ())
            # masked plan: the same two passes at the same places, through the *_kmask entries with the cross block's masks
            catt = lambda fn, fn_km: (fn, self.dtype, A(AttnProblem, t["c.att"])) if self._km_cross is None else \
                (fn_km, self.dtype, A(AttnProblem, t["c.att"]), self._km_cross)
            dq_step = catt(ops.attn_bwd_dq, ops.attn_bwd_dq_kmask)
            dkv = catt(ops.attn_bwd_dkv, ops.attn_bwd_dkv_kmask)
            # (bf16x3: the weight gradients are launched BEHIND the data-gradient products that split the same gradients --
            # dg_fc1 splits dh1, dg_q splits dq -- so that the side stream finds those images instead of splitting again)
            steps += [(WAIT, i + 2)] + ffn(t["f.grads"] + t["f.acts"] if x3 else (), x3) + \
                [nn(t["c.dgout"]), dq_step] + \
                ([] if lr else [(SIDE if self._dkv_side == "1" else SIDE2, dkv) if self._dkv_side in ("1", "2") else dkv]) + \
                ([] if x3 or lr else [wg_att]) + [nn(t["c.dgq"])] + ([wg_att] if x3 and not lr else [])
            # dK / dV (above) feed only side work: beside the main chain where the side stream has slack (see _DKV_SIDE_ENV)
            if c.biprojection:
                steps += [(ops.rows_cast, self.dtype, A(CastProblem, t["s.cast"]))] + self_half(())
            else:
                steps.append(ln(t["ln0"]))
            if lr:
                # low-rank key side: no dK / dV pass; the side stream continues from the dS / Pd the dQ pass wrote.  Issued
                # BEHIND the rest of the layer's main chain
                steps += [(SIDE, (ops.expand_heads, self.dtype, A(ExpandProblem, t["c.expand"]))), (SIDE, nn(t["c.lrqk"])), wg_att]
            # folded K/V gradients of this layer -> in_proj / LayerNorm parameter gradients; with it every gradient of
            # layer i is final once the side stream reaches MARK i and the main stream this point (all-reduce hook)
            store_dw = stores and not c.biprojection
            unfold = (ops.unfold_grads_ws,) + self._unfold[i] + (d, store_dw) if self.det else (ops.unfold_grads,) + self._unfold[i] + (store_dw,)
            steps += [(SIDE, unfold), (MARK, i)]
        if not self._kv:
            return steps + [JOIN]
        # d(khat), d(vhat): all layers' dK / dV against the stacked projection weights, one product over K = L ld per
        # encoder; then -> d(embedded key / value source): LayerNorm backward without affine
        hat, dg_kv = [], []
        for e, b in zip(self.encs, self.buf):
            if lr:                   # d(khat) of batch element bb = dS_all[:, bb]^T (Qexp W_k')_all[:, bb], K = layers H T
                KK, Sp = c.layers * c.H * e.T, b["Sp"]
                for mat, prod, G_ in ((b["dSall"], b["qkall"], b["Gk"]), (b["Pdall"], b["daall"], b["Gv"])):
                    dg_kv.append(ops.gemm_problem(mat, prod, G_, e.S, d, KK, self.B * Sp, self.B * self.ld, self.B * d,
                                                  batch=(self.B, Sp, self.ld, d)))
            else:
                for all_, stack, G_ in ((b["dkall"], KSTACK, b["Gk"]), (b["dvall"], VSTACK, b["Gv"])):
                    dg_kv.append(ops.gemm_problem(all_, st.sptr(e.prefix + stack), G_, b["Rk"], d, c.layers * self.ld, c.layers * self.ld,
                                                  self.ld, d))
            if not self._kv_fused:
                hat += [ops.ln_problem(b["ke"], self._ones, None, b["stk"][0], b["stk"][1], b["Rk"], dy=b["Gk"], ldy=d, dx=b["dke"]),
                        ops.ln_problem(b["ve"], self._ones, None, b["stv"][0], b["stv"][1], b["Rk"], dy=b["Gv"], ldy=d, dx=b["dve"])]
        # fused: LayerNorm backward + embedding backward (+ the sum of the two gradients) of every source in one launch
        last = (ops.kv_source_bwd, self._kvsrc[training], self.table, d, math.sqrt(d)) if self._kv_fused else ln(hat)
        return steps + [(SIDE, self._gemm(GEMM_TN if lr else GEMM_NN, dg_kv)), (SIDE, last), JOIN]

    @staticmethod
    def store_written(prefix: str, layers: int):
        """Names of the parameters whose gradient the `stores` tables write with a plain store (ParamStore.set_store_written)."""
        return [f"{prefix}layers.{i}.{leaf}" for i in range(layers)
                for leaf in ("self_attn.in_proj_weight", "self_attn.out_proj.weight", "fc1.weight", "fc2.weight")]

    def backward(self, douts: Sequence[Optional[torch.Tensor]], on_layer=None, stores: bool = False):
        """douts[e]: fp32 [T_e,B,d] gradient of encoder e's output (None = zero).  Returns the plan-owned
        gradients w.r.t. each encoder's query, key and value sources (three lists), and accumulates
        parameter gradients into the ParamStore's flat gradient buffer (stores=True: the large weight gradients are
        WRITTEN by their first launch -- the buffer was not cleared, ParamStore.begin_backward(stores=True))."""
        seed, training = self._last
        c, st, B, d = self.cfg, self.store, self.B, self.cfg.d
        fin, keep = [], []
        top = c.layers - 1
        self._acc0.zero_()
        for e, b, g in zip(self.encs, self.buf, douts):
            dx_top = b["dxg"] if b["tailp"] else b["dx"]          # gradient of the top layer's output rows
            if g is None:
                dx_top.zero_()
                b["dyf"][top % 3].zero_()
                continue
            if tuple(g.shape) != (b["Tl"][-1], B, d) or g.dtype != torch.float32:
                raise ValueError(f"encoder {e.prefix}: output gradient must be fp32 [{b['Tl'][-1]},{B},{d}], got {tuple(g.shape)} {g.dtype}")
            g = g.contiguous()
            keep.append(g)
            fin.append(ops.ln_problem(b["x"][c.layers], st.p(e.prefix + "layer_norm.weight"), None, b["stf"][0], b["stf"][1], b["Rl"][-1],
                                      dy=g, ldy=d, dx=dx_top, dgamma=st.gptr(e.prefix + "layer_norm.weight"),
                                      dbeta=st.gptr(e.prefix + "layer_norm.bias"),
                                      cast=b["dyf"][top % 3], ldc=self.ld,
                                      cast_colsum=self._bias_route(st.gptr(self._pn(e, top, "fc2.bias")))[0],
                                      drop_p=c.res_dropout if training else 0.0, drop_site=site(e.enc_id, top, S_RES2)))
        if fin:
            ops.ln_bwd(fin, d, self.dtype, seed, deterministic=self.det)
        # on_layer(i, events): every parameter gradient of layer i (and, with the first call, of the final LayerNorm)
        # is complete once `events` have passed -- the data-parallel exchange starts there (distributed.GradSync)
        self._run(self._bwd[(training, stores)], seed, on_layer)
        p = c.embed_dropout if training else 0.0
        emb = []
        for e, b in zip(self.encs, self.buf):
            emb.append(ops.embed_problem(b["dx"], b["dxq"], e.T, B, drop_p=p, drop_site=site(e.enc_id, 0, S_EMB_Q)))
            if self._kv and not self._kv_fused:
                emb.append(ops.embed_problem(b["dke"], b["dxk"], e.S, B, drop_p=p, drop_site=site(e.enc_id, 0, S_EMB_K)))
                emb.append(ops.embed_problem(b["dve"], b["dxv"], e.S, B, drop_p=p, drop_site=site(e.enc_id, 0, S_EMB_V)))
        ops.embed_pos_bwd(emb, d, math.sqrt(d), seed)
        return self.input_grads()

    def merge_kv_grads(self, dests: Optional[Sequence[Optional[torch.Tensor]]] = None) -> bool:
        """Opt in: backward() writes ONE gradient per key / value source, d(xk) + d(xv) summed in fp32 -- what a caller that
        passes the same tensor as xk and xv adds up anyway.  dests[e] (contiguous fp32 [S_e, B, d], 16-byte aligned; None:
        the plan's own buffer) receives encoder e's sum; input_grads() then returns it in the key list and None in the value
        list.  Only the fused key / value source launch can do this: returns False, and changes nothing, without it."""
        if not self._kv_fused:
            return False
        for i, (e, b) in enumerate(zip(self.encs, self.buf)):
            dst = dests[i] if dests is not None and dests[i] is not None else b["dxk"]
            if (tuple(dst.shape) != (e.S, self.B, self.cfg.d) or dst.dtype != torch.float32 or not dst.is_contiguous()
                    or dst.data_ptr() % 16):
                raise ValueError(f"encoder {e.prefix}: merged key / value gradient must be contiguous, 16-byte aligned fp32 "
                                 f"[{e.S},{self.B},{self.cfg.d}], got {tuple(dst.shape)} {dst.dtype}")
            self._kv_dst[i] = dst
            for arr in self._kvsrc.values():
                arr[i].dxk, arr[i].dxv = dst.data_ptr(), None
        return True

    def input_grads(self):
        """The plan-owned buffers backward() leaves the query, key and value source gradients in (three lists); after
        merge_kv_grads(): the merged gradient's tensor in the key list, None in the value list."""
        kv = lambda n: [b[n] if self._kv else None for b in self.buf]       # no key / value source: None in its place
        dk, dv = kv("dxk"), kv("dxv")
        for i, dst in enumerate(self._kv_dst):
            if dst is not None:
                dk[i], dv[i] = dst, None
        return [b["dxq"] for b in self.buf], dk, dv


KVF = "self_attn.in_proj_weight#kvf"      # key suffix of the folded key/value shadow and bias


KSTACK, VSTACK = "#kstack", "#vstack"     # per-encoder stacks of the folded key / value projection weights


def register_encoder_shadows(store: ParamStore, prefix: str, d: int, layers: int, biprojection: bool = False) -> None:
    lnK = 1 if biprojection else 0        # LayerNorm applied to the key / value source (transformer.py:167-172)
    ld = pad32(d)
    for i in range(layers):
        p = f"{prefix}layers.{i}."
        store.add_shadow(p + "self_attn.in_proj_weight", p + "self_attn.in_proj_weight", 3 * d, d)
        # key / value projections with that LayerNorm folded in: W' = W * gamma (columns), b' = W beta + b.  The layers' W'
        # are STACKED per encoder (block i = rows [i ld, i ld + d) of a [layers ld, ld] shadow, pad rows zero): layer i's
        # projection reads its block, and the key / value-side data gradient of ALL layers is one product over K = layers ld
        if i == 0:
            store.add_blank_shadow(prefix + KSTACK, layers * ld, ld)
            store.add_blank_shadow(prefix + VSTACK, layers * ld, ld)
        store.add_shadow(p + KVF + ".k", p + "self_attn.in_proj_weight", d, d, src_row0=d, colscale=p + f"layer_norms.{lnK}.weight",
                         base_key=prefix + KSTACK, dst_row0=i * ld)
        store.add_shadow(p + KVF + ".v", p + "self_attn.in_proj_weight", d, d, src_row0=2 * d, colscale=p + f"layer_norms.{lnK}.weight",
                         base_key=prefix + VSTACK, dst_row0=i * ld)
        store.add_fold(p + KVF, p + "self_attn.in_proj_weight", d, 2 * d, d, p + f"layer_norms.{lnK}.bias",
                       p + "self_attn.in_proj_bias", d)
        store.add_shadow(p + "self_attn.out_proj.weight", p + "self_attn.out_proj.weight", d, d)
        store.add_shadow(p + "fc1.weight", p + "fc1.weight", 4 * d, d)
        store.add_shadow(p + "fc2.weight", p + "fc2.weight", d, 4 * d)
