"""Evaluation on the HIP path: what the reference's model_eval (train.py:165-280) collects and computes, kept on the device.

`Evaluator.update` appends one batch's predictions, scores, targets and loss to a device store in one launch -- no host
read, no torch compute op -- so the captured graphs of the next forward queue behind the current one.  `compute` runs
bpm_eval_finalize and reads one small buffer: the evaluation's single synchronisation.  It returns the PRIMITIVES (counts,
F1 / average precision in every averaging, the regression sums' metrics); training.model_eval arranges them into the
reference's dict.  No scikit-learn: average precision is computed from integer rank counts (csrc/eval.hip, DESIGN.md
section 5), bit-reproducible.  There is no CPU path.

Under data parallelism each rank fills its own Evaluator from a share of the batches; `all_gather` (pack, one integer
all_reduce, merge -- all on the device) leaves the store of the whole evaluation on every rank, bit for bit.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, ops

KINDS = {"multilabel": _lib.EVAL_MULTILABEL, "regression": _lib.EVAL_REGRESSION, "classes": _lib.EVAL_CLASSES}
# gate dtypes by the code that all_gather exchanges
_GATE_DTYPES = (torch.float32, torch.float16, torch.bfloat16, torch.float64, torch.uint8, torch.int8, torch.int16, torch.int32,
                torch.int64, torch.bool)


def weighted_accuracy(tp, fp, fn, tn):
    """weighted_acc of the reference (train.py:138-163) from a class's counts: wacc = (tp n / p + tn) / (2 n) with
    p = tp + fn positives and n = tn + fp negatives, and the F1 with the reference's 1e-8 terms.  n = 0 or p = 0 gives NaN
    here; the reference raises ZeroDivisionError there."""
    tp, fp, fn, tn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn, tn))
    p, n = tp + fn, tn + fp
    with np.errstate(divide="ignore", invalid="ignore"):
        wacc = np.where((p > 0) & (n > 0), (tp * n / p + tn) / (2 * n), np.nan)
    recall = tp / (tp + fn + 1e-8)
    precision = tp / (tp + fp + 1e-8)
    f1 = 2 * recall * precision / (recall + precision + 1e-8)
    return wacc, np.where((p > 0) & (n > 0), f1, np.nan)


def _f1(tp, fp, fn):
    tp, fp, fn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn))
    den = 2.0 * tp + fp + fn
    return np.where(den > 0, 2.0 * tp / np.where(den > 0, den, 1.0), 0.0)      # scikit-learn's zero_division: 0


class Evaluator:
    """Device-side store and metrics of one evaluation.

    kind: "multilabel" (BCE tasks: logits [B, C], fp32 0/1 targets [B, C]), "regression" (cmu-mosi: logits [B] or [B, 1],
    fp32 targets [B]) or "classes" (cross-entropy tasks: logits [B, C], int64 targets [B]).  capacity: the most rows one
    evaluation holds; max_batches: the most update calls (default: capacity)."""

    def __init__(self, kind: str, num_classes: int, capacity: int, max_batches: Optional[int] = None, device="cuda"):
        if kind not in KINDS:
            raise ValueError(f"kind: expected one of {sorted(KINDS)}, got {kind!r}")
        if kind == "regression" and num_classes != 1:
            raise ValueError(f"num_classes: a regression evaluator has one output, got {num_classes}")
        if num_classes < 1 or capacity < 1:
            raise ValueError(f"num_classes / capacity: must be at least 1, got {num_classes} / {capacity}")
        max_batches = capacity if max_batches is None else max_batches
        if max_batches < 1:
            raise ValueError(f"max_batches: must be at least 1, got {max_batches}")
        device = torch.device(device)
        if device.type != "cuda":
            raise RuntimeError("Evaluator: needs a CUDA (HIP) device; there is no CPU path")
        self.kind, self.C, self.capacity, self.max_batches, self.device = kind, num_classes, capacity, max_batches, device
        k, Cn = KINDS[kind], num_classes
        nws = ops.eval_ws_bytes(k, capacity, Cn)
        if nws == 0:
            raise ValueError(f"capacity: {capacity} rows of {Cn} classes are more than one evaluation store holds (2^31 elements)")
        new = lambda shape, dt: torch.zeros(shape, device=device, dtype=dt)       # noqa: E731
        ml = kind == "multilabel"
        self._score = new((capacity, Cn) if ml else (capacity,), torch.float32) if kind != "classes" else None
        self._pred = new((capacity, Cn), torch.uint8) if ml else None
        self._label = new((capacity, Cn) if ml else (capacity,), torch.uint8) if kind != "regression" else None
        self._predict = None if ml else new((capacity,), torch.float32)
        self._raw = new((capacity,), torch.float32) if kind == "regression" else None
        self._target = None if ml else new((capacity,), torch.float32)
        self._losses = new((max_batches,), torch.float32)
        # result (fp64), counts (int64) and the counter of refused targets (int32) in ONE buffer: one copy reads them all
        self._nres, self._ncnt = (Cn + 4, 4 * Cn + 1) if ml else (7, 8)
        self._out = new((self._nres + self._ncnt + 1,), torch.int64)
        self._result = self._out[:self._nres].view(torch.float64)
        self._counts = self._out[self._nres:self._nres + self._ncnt]
        self._bad = self._out[self._nres + self._ncnt:].view(torch.int32)
        self._ws = new(((nws + 7) // 8,), torch.int64)
        self._desc = ops.eval_desc(k, Cn, capacity, max_batches=max_batches, score=self._score, predict=self._predict, raw=self._raw,
                                   target=self._target, pred=self._pred, label=self._label, losses=self._losses, bad=self._bad,
                                   result=self._result, counts=self._counts, ws=self._ws)
        self._gates: Optional[torch.Tensor] = None
        self.n = self.nbatches = self.nlosses = 0

    def reset(self) -> None:
        """Forget the stored rows (the buffers are kept)."""
        self.n = self.nbatches = self.nlosses = 0
        self._gates = None
        self._bad.zero_()

    # ------------------------------------------------------------------
    def _check(self, name: str, t, dtype, shapes) -> None:
        if not isinstance(t, torch.Tensor):
            raise ValueError(f"{name}: expected a tensor, got {type(t).__name__}")
        if t.dtype != dtype:
            raise ValueError(f"{name}: expected {dtype}, got {t.dtype}")
        if tuple(t.shape) not in shapes:
            raise ValueError(f"{name}: shape {tuple(t.shape)}, expected " + " or ".join(str(list(s)) for s in shapes))
        if not t.is_cuda:
            raise RuntimeError(f"{name}: the evaluator needs CUDA (HIP) tensors; there is no CPU path")
        if t.dim() == 2 and t.shape[0] > 1 and t.stride(-1) != 1 and t.shape[-1] > 1:
            raise ValueError(f"{name}: the last dimension must have unit stride, got strides {t.stride()}")

    def update(self, logits: torch.Tensor, target: torch.Tensor, loss: Optional[torch.Tensor] = None,
               gates: Optional[torch.Tensor] = None) -> None:
        """Append one batch: no host synchronisation, no torch compute op.  loss: the batch's criterion value, a 0-dim (or
        one-element) fp32 device tensor; gates [B, n d]: kept on the device for predictions()."""
        if not isinstance(logits, torch.Tensor) or logits.dim() not in (1, 2) or logits.shape[0] < 1:
            raise ValueError(f"logits: expected [B, {self.C}]" + (" or [B]" if self.kind == "regression" else "") + " with B >= 1")
        B = logits.shape[0]
        if self.kind == "regression":
            self._check("logits", logits, torch.float32, ((B,), (B, 1)))
            self._check("target", target, torch.float32, ((B,),))
            ld = logits.stride(0) if B > 1 else 1
            if target.stride(0) != 1 and B > 1:
                raise ValueError(f"target: must be contiguous, got strides {target.stride()}")
            ldt = 1
        else:
            self._check("logits", logits, torch.float32, ((B, self.C),))
            ld = logits.stride(0) if B > 1 else self.C
            if ld < self.C:
                raise ValueError(f"logits: row stride {ld} is less than the {self.C} classes")
            if self.kind == "multilabel":
                self._check("target", target, torch.float32, ((B, self.C),))
                ldt = target.stride(0) if B > 1 else self.C
                if ldt < self.C:
                    raise ValueError(f"target: row stride {ldt} is less than the {self.C} classes")
            else:
                self._check("target", target, torch.int64, ((B,),))
                if target.stride(0) != 1 and B > 1:
                    raise ValueError(f"target: must be contiguous, got strides {target.stride()}")
                ldt = 0
        if loss is not None:
            self._check("loss", loss, torch.float32, ((), (1,)))
            if self.nlosses != self.nbatches:
                raise ValueError("loss: given for this batch but not for an earlier one of the same evaluation")
        elif self.nlosses:
            raise ValueError("loss: missing for this batch but given for an earlier one of the same evaluation")
        if self.n + B > self.capacity:
            raise ValueError(f"capacity: {self.n} rows stored + {B} exceed the capacity of {self.capacity}")
        if self.nbatches + 1 > self.max_batches:
            raise ValueError(f"max_batches: this is batch {self.nbatches + 1} of at most {self.max_batches}")
        if gates is not None:
            if not isinstance(gates, torch.Tensor) or gates.dim() != 2 or gates.shape[0] != B or not gates.is_cuda:
                raise ValueError(f"gates: expected a device tensor [B = {B}, n d]")
            if self._gates is None:
                if self.n:
                    raise ValueError("gates: given for this batch but not for an earlier one of the same evaluation")
                self._gates = torch.empty((self.capacity, gates.shape[1]), device=self.device, dtype=gates.dtype)
            elif self._gates.shape[1] != gates.shape[1] or self._gates.dtype != gates.dtype:
                raise ValueError(f"gates: [B, {gates.shape[1]}] {gates.dtype} after [B, {self._gates.shape[1]}] {self._gates.dtype}")
            self._gates[self.n:self.n + B].copy_(gates)
        elif self._gates is not None:
            raise ValueError("gates: missing for this batch but given for an earlier one of the same evaluation")
        with torch.cuda.device(self.device):
            ops.eval_update(self._desc, logits, target, B, self.n, ld=ld, ldt=ldt, loss=loss, batch_index=self.nbatches)
        self.n += B
        self.nbatches += 1
        self.nlosses += loss is not None

    # ------------------------------------------------------------------
    # sharded evaluation: every rank fills its own store from a contiguous share of the batches, the shards are exchanged
    # as images of 32-bit words and merged on the device in rank order (csrc/eval.hip)
    def pack(self, rows: Optional[int] = None, batches: Optional[int] = None, out: Optional[torch.Tensor] = None) -> torch.Tensor:
        """The exchange image of the stored rows, their losses and the counter of refused targets: an int32 device tensor
        laid out for a shard of up to `rows` rows and `batches` losses (default: what is stored), zero past the stored
        data.  out: an int32 tensor to write it to (every element is written).  One launch, no host read."""
        rows = self.n if rows is None else rows
        batches = self.nlosses if batches is None else batches
        if rows < self.n or batches < self.nlosses:
            raise ValueError(f"pack: an image for {rows} rows / {batches} losses cannot hold the {self.n} / {self.nlosses} stored")
        nbytes = ops.eval_image_bytes(KINDS[self.kind], rows, batches, self.C)
        if nbytes == 0:
            raise ValueError(f"pack: no image holds {rows} rows of {self.C} classes and {batches} losses")
        if out is None:
            out = torch.empty((nbytes // 4,), device=self.device, dtype=torch.int32)
        with torch.cuda.device(self.device):
            ops.eval_pack(self._desc, self.n, self.nlosses, out, rows=rows, batches=batches)
        return out

    def _shard_counts(self, rows, batches, losses=None):
        """Per-rank rows / update calls / losses as int lists, refused where the merged evaluation would not fit or would
        carry losses for some batches only."""
        rows, batches = [int(v) for v in rows], [int(v) for v in batches]
        losses = list(batches) if losses is None else [int(v) for v in losses]
        W = len(rows)
        if not 1 <= W <= _lib.EVAL_MAX_RANKS or len(batches) != W or len(losses) != W:
            raise ValueError(f"merge: 1 to {_lib.EVAL_MAX_RANKS} shards with one row, batch and loss count each, got "
                             f"{W} / {len(batches)} / {len(losses)}")
        if min(rows) < 0 or min(batches) < 0 or min(losses) < 0:
            raise ValueError(f"merge: negative counts in rows {rows}, batches {batches}, losses {losses}")
        if sum(rows) > self.capacity:
            raise ValueError(f"capacity: the shards hold {sum(rows)} rows, the capacity is {self.capacity}")
        if sum(batches) > self.max_batches:
            raise ValueError(f"max_batches: the shards hold {sum(batches)} batches of at most {self.max_batches}")
        if any(l not in (0, b) for l, b in zip(losses, batches)) or (any(losses) and losses != batches):
            raise ValueError(f"loss: given for some batches only (batches {batches}, losses {losses})")
        return rows, batches, losses

    def merge(self, images: torch.Tensor, rows, batches, losses=None) -> None:
        """Fill the store from W images (int32 [W, words], each laid out for max(rows) rows and max(losses) losses, as
        pack(max(rows), max(losses)) writes them): shard r's rows go behind those of the shards before it, in order, and
        so do its losses; the counters of refused targets add.  rows / batches / losses: per shard, the rows, the update
        calls and the losses it carries (default: one per update call; all or none of the batches carry one).  Sets n,
        nbatches and nlosses; gates are not part of an image (all_gather moves them).  This evaluator's own image may be
        among the sources.  One launch, no host read; a refusal leaves the store as it was."""
        rows, batches, losses = self._shard_counts(rows, batches, losses)
        if not isinstance(images, torch.Tensor) or images.dtype != torch.int32 or images.dim() != 2 or images.shape[0] != len(rows):
            raise ValueError(f"images: expected an int32 tensor [{len(rows)}, words]")
        if not images.is_cuda:
            raise RuntimeError("images: the evaluator needs CUDA (HIP) tensors; there is no CPU path")
        need = ops.eval_image_bytes(KINDS[self.kind], max(rows), max(losses), self.C) // 4
        if images.shape[1] < need:
            raise ValueError(f"images: {images.shape[1]} words each, shards of up to {max(rows)} rows and {max(losses)} losses take {need}")
        with torch.cuda.device(self.device):
            ops.eval_merge(self._desc, images.contiguous(), rows, losses)
        self.n, self.nbatches, self.nlosses = sum(rows), sum(batches), sum(losses)

    def all_gather(self, process_group=None, counts=None, gates: Optional[bool] = None) -> None:
        """The collective step of a sharded evaluation: pack this rank's shard, exchange the images, merge them in rank
        order into every rank's store.  Afterwards compute() and predictions() behave on every rank as on one evaluator
        that was fed all batches in order, bit for bit.  Without an initialised process group, or in a world of one, a
        no-op.

        counts: per rank (rows, batches) or (rows, batches, losses) -- losses default to batches -- when every rank knows
        them already (from the shapes of a batch list that all ranks share).  Then nothing is read on the host, and kind,
        C, the capacities and whether gates are kept are the caller's promise to be alike on all ranks.  Without counts
        -- or when a rank holds no rows, which then cannot know whether the others keep gates -- rows, batches, losses,
        kind, C, capacities and the gates' width and dtype are exchanged first: ONE SMALL HOST READ per evaluation, and a
        mismatch raises ValueError on every rank alike.

        The images travel at one common size (the largest shard's) as an int32 [W, words] buffer that is zero outside the
        own slot, summed by all_reduce -- exact for every bit pattern, and served for device tensors by nccl and gloo
        alike.  Gates, when kept, follow in a second all_reduce of their bytes, dtype and bits unchanged.  Every rank
        issues the same collectives in the same order whatever its shard holds.

        gates: whether the evaluation keeps gates, when the caller knows (model_eval passes its output_gates), so that no
        rank decides on the second collective from what it happens to hold: False -- none, with counts no host read; True
        -- the gates' width and dtype are exchanged with the counts (the host read above) and a rank with rows but
        without gates makes every rank raise.  None: as this rank holds them, which with counts given is once more the
        caller's promise.

        A rank that finds its own shard is not what `counts` (or gates = False) promised still takes part in every
        collective, with a voided image in place of its shard, and raises ValueError afterwards.  The other ranks cannot
        raise at once without a host read; their merged store is INVALID (the voided shard's rows are zeros), its counter
        of refused targets reads -1, and their compute() raises ValueError on it; predictions() must not be used then."""
        import torch.distributed as dist
        if not (dist.is_available() and dist.is_initialized()):
            return
        W = dist.get_world_size(process_group)
        if W == 1:
            return
        rank = dist.get_rank(process_group)
        if counts is not None:
            counts = [tuple(int(v) for v in c) for c in counts]
            if len(counts) != W or any(len(c) not in (2, 3) for c in counts):
                raise ValueError(f"counts: expected {W} entries (rows, batches[, losses]), got {counts}")
            counts = [c if len(c) == 3 else c + (c[1],) for c in counts]
        kept = self._gates is not None
        mine = (self.n, self.nbatches, self.nlosses)
        late = None                      # an error only this rank knows of: raised after the collectives, never in their place
        with torch.cuda.device(self.device):
            if counts is not None and all(c[0] > 0 for c in counts) and gates is not True:
                rows, batches, losses = self._shard_counts(*zip(*counts))
                if counts[rank] != mine:
                    late = f"counts: rank {rank} was promised as (rows, batches, losses) = {counts[rank]} and holds {mine}"
                elif gates is False and kept:
                    late = f"gates: rank {rank} keeps gates in an all_gather that was told there are none"
                gates = kept if gates is None else False
                gate_width, gate_dtype = (self._gates.shape[1], self._gates.dtype) if gates else (0, None)
            else:
                meta = mine + (KINDS[self.kind], self.C, self.capacity, self.max_batches, int(kept),
                               self._gates.shape[1] if kept else 0, _GATE_DTYPES.index(self._gates.dtype) if kept else 0)
                table = torch.zeros((W, len(meta)), device=self.device, dtype=torch.int64)
                table[rank] = torch.tensor(meta, dtype=torch.int64)
                dist.all_reduce(table, op=dist.ReduceOp.SUM, group=process_group)
                table = table.cpu().tolist()                                           # the one host read
                if any(t[3:5] != table[0][3:5] for t in table):
                    raise ValueError(f"all_gather: kind / C differ between ranks: {[tuple(t[3:5]) for t in table]}")
                if any(t[5:7] != table[0][5:7] for t in table):
                    raise ValueError(f"all_gather: capacity / max_batches differ between ranks: {[tuple(t[5:7]) for t in table]}")
                if counts is not None and [tuple(t[:3]) for t in table] != counts:
                    raise ValueError(f"counts: given {counts}, the ranks hold {[tuple(t[:3]) for t in table]}")
                rows, batches, losses = self._shard_counts(*zip(*(t[:3] for t in table)))
                holders = [t for t in table if t[0] > 0]
                if any(t[7:] != holders[0][7:] for t in holders):
                    raise ValueError(f"gates: kept on some ranks only, or of different width / dtype: {[tuple(t[7:]) for t in table]}")
                found = bool(holders) and bool(holders[0][7])
                if gates is not None and holders and gates != found:
                    raise ValueError(f"gates: all_gather was told gates = {gates}, the ranks with rows say {found}")
                gates = found
                gate_width, gate_dtype = (holders[0][8], _GATE_DTYPES[holders[0][9]]) if gates else (0, None)
            k, rmax, bmax = KINDS[self.kind], max(rows), max(losses)
            images = torch.zeros((W, ops.eval_image_bytes(k, rmax, bmax, self.C) // 4), device=self.device, dtype=torch.int32)
            if late is None:
                self.pack(rmax, bmax, out=images[rank])
            else:
                images[rank, 1] = 1      # the void mark: every rank's merge leaves bad = -1 and its compute() raises
            dist.all_reduce(images, op=dist.ReduceOp.SUM, group=process_group)
            if gates:
                slots = torch.zeros((W, self.gate_slot_bytes(rmax, gate_width, gate_dtype)), device=self.device, dtype=torch.uint8)
                if late is None:
                    self.pack_gates(slots[rank])
                dist.all_reduce(slots.view(torch.int32), op=dist.ReduceOp.SUM, group=process_group)
            if late is not None:
                raise ValueError(late)
            self.merge(images, rows, batches, losses)
            if gates:
                self.merge_gates(slots, rows, gate_width, gate_dtype)

    @staticmethod
    def gate_slot_bytes(rows: int, width: int, dtype: torch.dtype) -> int:
        """Bytes of one rank's slot in the gates exchange: `rows` rows of `width` gates, rounded up to 8."""
        return (rows * width * dtype.itemsize + 7) // 8 * 8

    def pack_gates(self, out: torch.Tensor) -> None:
        """The kept gates of the stored rows as bytes into the head of `out` (uint8, a slot of gate_slot_bytes that is zero
        elsewhere); nothing when no gates are kept or no rows stored."""
        if self._gates is not None and self.n:
            flat = self._gates[:self.n].reshape(-1).view(torch.uint8)
            out[:flat.numel()] = flat

    def merge_gates(self, slots: torch.Tensor, rows, width: int, dtype: torch.dtype) -> None:
        """Lay the gates of W shards (uint8 [W, slot bytes], as pack_gates fills them) behind each other in shard order,
        dtype and bits unchanged: shard r's rows go to rows [sum(rows[:r]), ...), where merge() puts its predictions."""
        if self._gates is None:
            self._gates = torch.empty((self.capacity, width), device=self.device, dtype=dtype)
        elif self._gates.shape[1] != width or self._gates.dtype != dtype:
            raise ValueError(f"gates: [B, {width}] {dtype} into kept gates [B, {self._gates.shape[1]}] {self._gates.dtype}")
        if sum(rows) > self.capacity:
            raise ValueError(f"capacity: the shards hold {sum(rows)} rows, the capacity is {self.capacity}")
        r0, row_bytes = 0, width * dtype.itemsize
        for r, nr in enumerate(rows):
            if nr:
                self._gates[r0:r0 + nr] = slots[r, :nr * row_bytes].view(dtype).view(nr, width)
            r0 += nr

    # ------------------------------------------------------------------
    def compute(self) -> dict:
        """Finalize on the device and read the result buffer once (the evaluation's one sync).  Returns Python numbers and
        numpy arrays.  Every kind: `loss` (mean of the batch losses, NaN for none), `n`, `bad` (targets refused: neither 0
        nor 1 / class index outside [0, C)).

        multilabel: `tp`, `fp`, `fn`, `tn` (int64 [C]); `f1` {class, macro, micro, weighted (by support), samples};
        `subset_accuracy`; `ap` {class, macro, micro, samples}; `wacc`, `wf1` ([C], see weighted_accuracy: NaN where the
        reference raises ZeroDivisionError).
        regression / classes: `mae`, `corr`, `accuracy_7`, `accuracy_2`, `weighted_f1`, `acc` over the rows that take part
        (`n`).  `weighted_f1` weights the two classes' F1 by the supports of the PREDICTIONS: the reference calls
        f1_score(binary_preds, binary_truth, average='weighted') with the predictions first (train.py:268)."""
        if self.n < 1:
            raise ValueError("compute: no rows stored")
        with torch.cuda.device(self.device):
            ops.eval_finalize(self._desc, self.n, self.nlosses)
        host = self._out.cpu().numpy()
        res = host[:self._nres].view(np.float64)
        cnt = host[self._nres:self._nres + self._ncnt].astype(np.int64)
        bad = int(host[self._nres + self._ncnt:].view(np.int32)[0])
        if bad < 0:
            raise ValueError("compute: a rank voided its shard in all_gather (it held other rows, batches or gates than all ranks were "
                             "promised; that rank has raised): the merged store is invalid")
        out = {"loss": float(res[0]), "bad": bad}
        if self.kind == "multilabel":
            Cn = self.C
            k = cnt[:4 * Cn].reshape(Cn, 4)
            tp, fp, fn, tn = (k[:, i].copy() for i in range(4))
            f1c = _f1(tp.astype(np.float64), fp, fn)
            sup = (tp + fn).astype(np.float64)
            wacc, wf1 = weighted_accuracy(tp, fp, fn, tn)
            apc = res[1:1 + Cn].copy()
            out.update(n=self.n, tp=tp, fp=fp, fn=fn, tn=tn,
                       f1={"class": f1c, "macro": float(f1c.mean()), "micro": float(_f1(float(tp.sum()), fp.sum(), fn.sum())),
                           "weighted": float((f1c * sup).sum() / sup.sum()) if sup.sum() > 0 else 0.0, "samples": float(res[3 + Cn])},
                       subset_accuracy=int(cnt[4 * Cn]) / self.n,
                       ap={"class": apc, "macro": float(apc.mean()), "micro": float(res[1 + Cn]), "samples": float(res[2 + Cn])},
                       wacc=wacc, wf1=wf1)
            return out
        n = int(cnt[6])
        sad, sp, st, spp, stt, spt = (float(v) for v in res[1:7])
        a, b, c, d = (float(v) for v in cnt[1:5])            # p > 0 and t > 0, p only, t only, neither
        nz = a + b + c + d
        with np.errstate(divide="ignore", invalid="ignore"):
            den = np.sqrt(np.float64(n * spp - sp * sp) * np.float64(n * stt - st * st))
            corr = float(np.float64(n * spt - sp * st) / den)
            wf = float((np.float64(a + b) * _f1(a, b, c) + np.float64(c + d) * _f1(d, c, b)) / np.float64(nz))
            out.update(n=n, mae=float(np.float64(sad) / n), corr=corr, accuracy_7=float(np.float64(cnt[0]) / n),
                       accuracy_2=float(np.float64(a + d) / nz), weighted_f1=wf, acc=float(np.float64(cnt[5]) / n))
        return out

    def predictions(self):
        """(targets, preds, scores[, gates]) of the stored rows as host arrays, what the reference hands to
        store_preds_to_disk.  multilabel: fp32 0/1 targets, bool predictions, fp32 sigmoid scores, all [N, C]; regression:
        targets, sigmoid predictions, raw logits [N]; classes: int64 targets and argmax predictions [N], scores None (the
        reference keeps the softmax, which is not stored here)."""
        n = self.n
        if self.kind == "multilabel":
            r = (self._label[:n].cpu().numpy().astype(np.float32), self._pred[:n].cpu().numpy().astype(bool), self._score[:n].cpu().numpy())
        elif self.kind == "regression":
            r = (self._target[:n].cpu().numpy(), self._score[:n].cpu().numpy(), self._raw[:n].cpu().numpy())
        else:
            r = (self._target[:n].cpu().numpy().astype(np.int64), self._predict[:n].cpu().numpy().astype(np.int64), None)
        return r + (self._gates[:n].cpu().numpy(),) if self._gates is not None else r
