"""Evaluation on the HIP path: what the reference's model_eval (train.py:165-280) collects and computes, kept on the device.

`Evaluator.update` appends one batch's predictions, scores, targets and loss to a device store in one launch -- no host
read, no torch compute op -- so the captured graphs of the next forward queue behind the current one.  `compute` runs
bpm_eval_finalize and reads one small buffer: the evaluation's single synchronisation.  It returns the PRIMITIVES (counts,
F1 / average precision in every averaging, the regression sums' metrics); training.model_eval arranges them into the
reference's dict.  No scikit-learn: average precision is computed from integer rank counts (csrc/eval.hip, DESIGN.md
section 5), bit-reproducible.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import numpy as np
import torch

from . import _lib, ops

KINDS = {"multilabel": _lib.EVAL_MULTILABEL, "regression": _lib.EVAL_REGRESSION, "classes": _lib.EVAL_CLASSES}


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
