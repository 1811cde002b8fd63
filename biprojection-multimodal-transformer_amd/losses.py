"""The training criterion on the HIP path: drop-in subclasses of the three torch modules the reference's get_criterion
builds (train.py:99-120) and calls at train.py:333.  `forward` is ONE autograd node: bpm_loss_fwd writes the loss and the
derivative for an upstream gradient of 1, bpm_loss_bwd scales that derivative by the upstream gradient, which it reads
on the device (`(loss / gradient_accumulation_steps).backward()` costs no host read).  Elements are carried in fp64 and
rounded once, sums run in a fixed order: loss and gradient are bitwise reproducible (csrc/loss.hip).

What torch's modules accept and these refuse (ValueError naming the argument): the per-element `weight` of BCE,
`label_smoothing`, class-probability targets and inputs other than [B, C] for cross-entropy, broadcasting between input
and target, a target that requires grad.  There is no CPU path.
"""
from __future__ import annotations

from typing import Optional

import torch
from torch.autograd.function import once_differentiable

from . import _lib, ops

_REDUCTIONS = {"mean": _lib.LOSS_MEAN, "sum": _lib.LOSS_SUM, "none": _lib.LOSS_NONE}


class _Criterion(torch.autograd.Function):
    """x fp32 [B, C] (unit column stride), target fp32 [B, C] contiguous or int64 [B]; returns the loss as the kernel
    leaves it: 0-dim for mean / sum, [B, C] or [B] for none."""

    @staticmethod
    def forward(ctx, x, target, weight, kind, reduction, ignore_index, bad, want_grad):
        B, Cn = x.shape
        with torch.cuda.device(x.device):
            if reduction == _lib.LOSS_NONE:
                loss = x.new_empty((B,) if kind == _lib.LOSS_CE else (B, Cn))
            else:
                loss = x.new_empty(())
            du = x.new_empty((B, Cn)) if want_grad else None
            nws = ops.loss_ws_bytes(kind, reduction, B, Cn)
            ws = torch.empty((nws + 7) // 8, device=x.device, dtype=torch.float64) if nws else None
            prob = ops.loss_problem(kind, reduction, x, target, loss, B, Cn, ld=x.stride(0) if B > 1 else Cn,
                                    ldt=None if kind == _lib.LOSS_CE or B == 1 else target.stride(0), weight=weight,
                                    ignore_index=ignore_index, dlogits_unit=du, bad=bad, ws=ws)
            ops.loss_fwd(prob)
        ctx.prob, ctx.du = prob, du          # prob is read for its sizes and dlogits_unit only: du keeps that pointer alive
        return loss

    @staticmethod
    @once_differentiable
    def backward(ctx, g):
        if ctx.du is None:
            raise RuntimeError("criterion: the forward ran without a gradient request (torch.no_grad or logits that did not require grad)")
        g = g.to(torch.float32).contiguous()
        dl = torch.empty_like(ctx.du)
        with torch.cuda.device(dl.device):
            ops.loss_bwd(ctx.prob, g, dl)
        return dl, None, None, None, None, None, None, None


def _reduction(name: str) -> int:
    if name not in _REDUCTIONS:
        raise ValueError(f"reduction: expected 'mean', 'sum' or 'none', got {name!r}")
    return _REDUCTIONS[name]


def _check_common(what: str, input: torch.Tensor, target: torch.Tensor) -> None:
    if target.requires_grad:
        raise ValueError(f"{what}: target requires grad; the HIP criterion differentiates with respect to the input only")
    if not input.is_floating_point():
        raise ValueError(f"{what}: input must be a floating-point tensor, got {input.dtype}")


def _no_cpu(what: str, *tensors) -> None:
    if not all(t.is_cuda for t in tensors if t is not None):
        raise RuntimeError(f"{what}: the HIP criterion needs CUDA (HIP) tensors; there is no CPU path")


def _rows(t: torch.Tensor) -> torch.Tensor:
    """Any shape -> fp32 [rows, last dim] with unit column stride (a view where torch can make one)."""
    t = t.to(torch.float32)
    t = t.reshape(1, 1) if t.dim() == 0 else t.reshape(-1, t.shape[-1])
    return t if t.stride(1) == 1 and (t.shape[0] == 1 or t.stride(0) >= t.shape[1]) else t.contiguous()


def _elementwise(what: str, kind: int, reduction: str, input: torch.Tensor, target: torch.Tensor, weight: Optional[torch.Tensor]):
    red = _reduction(reduction)
    _check_common(what, input, target)
    if input.shape != target.shape:
        raise ValueError(f"{what}: target of shape {tuple(target.shape)} against input of shape {tuple(input.shape)}; "
                         "the HIP criterion does not broadcast")
    if not target.is_floating_point():
        raise ValueError(f"{what}: target must be a floating-point tensor, got {target.dtype}")
    if input.numel() == 0:
        raise ValueError(f"{what}: input is empty")
    last = input.shape[-1] if input.dim() else 1
    if weight is not None and tuple(weight.shape) != (last,):
        raise ValueError(f"{what}: pos_weight of shape {tuple(weight.shape)}, expected [{last}] (the input's last dimension)")
    _no_cpu(what, input, target, weight)
    x, y = _rows(input), _rows(target).contiguous()
    if weight is not None:
        weight = weight.detach().to(torch.float32).contiguous()
    out = _Criterion.apply(x, y, weight, kind, red, 0, None, x.requires_grad and torch.is_grad_enabled())
    if red == _lib.LOSS_NONE:
        out = out.reshape(input.shape)
    return out.to(input.dtype)


class BCEWithLogitsLoss(torch.nn.BCEWithLogitsLoss):
    """nn.BCEWithLogitsLoss(pos_weight=...) on the HIP path; `pos_weight` is a buffer of shape [C] as in torch."""

    def __init__(self, pos_weight: Optional[torch.Tensor] = None, reduction: str = "mean", weight: Optional[torch.Tensor] = None):
        if weight is not None:
            raise ValueError("weight: the per-element rescaling weight of BCEWithLogitsLoss is not supported (pos_weight is)")
        _reduction(reduction)
        super().__init__(reduction=reduction, pos_weight=pos_weight)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        if self.weight is not None:
            raise ValueError("weight: the per-element rescaling weight of BCEWithLogitsLoss is not supported (pos_weight is)")
        return _elementwise("BCEWithLogitsLoss", _lib.LOSS_BCE, self.reduction, input, target, self.pos_weight)


class L1Loss(torch.nn.L1Loss):
    """nn.L1Loss on the HIP path (the reference's cmu-mosi criterion: [B] against [B])."""

    def __init__(self, reduction: str = "mean"):
        _reduction(reduction)
        super().__init__(reduction=reduction)

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        return _elementwise("L1Loss", _lib.LOSS_L1, self.reduction, input, target, None)


class CrossEntropyLoss(torch.nn.CrossEntropyLoss):
    """nn.CrossEntropyLoss(weight=..., ignore_index=...) over [B, C] logits and int64 [B] class indices on the HIP path.

    `bad_targets`: int32 device counter (None before the first forward) of class indices that were neither ignore_index
    nor in [0, C).  Such a row is treated exactly like an ignored row -- torch's kernel device-asserts on it.  The
    counter is cumulative and reading it is the caller's sync."""

    def __init__(self, weight: Optional[torch.Tensor] = None, ignore_index: int = -100, reduction: str = "mean",
                 label_smoothing: float = 0.0):
        if label_smoothing != 0:
            raise ValueError("label_smoothing: not supported by the HIP criterion (must be 0)")
        _reduction(reduction)
        super().__init__(weight=weight, ignore_index=ignore_index, reduction=reduction)
        self.bad_targets: Optional[torch.Tensor] = None

    def forward(self, input: torch.Tensor, target: torch.Tensor) -> torch.Tensor:
        what = "CrossEntropyLoss"
        red = _reduction(self.reduction)
        if self.label_smoothing != 0:
            raise ValueError("label_smoothing: not supported by the HIP criterion (must be 0)")
        _check_common(what, input, target)
        if input.dim() != 2 or input.shape[0] < 1 or input.shape[1] < 1:
            raise ValueError(f"{what}: input of shape {tuple(input.shape)}; the HIP criterion takes [B, C] logits")
        if target.is_floating_point() or target.is_complex():
            raise ValueError(f"{what}: target of dtype {target.dtype}; class-probability targets are not supported, pass class indices")
        if tuple(target.shape) != (input.shape[0],):
            raise ValueError(f"{what}: target of shape {tuple(target.shape)}, expected [{input.shape[0]}] class indices")
        if self.weight is not None and tuple(self.weight.shape) != (input.shape[1],):
            raise ValueError(f"{what}: weight of shape {tuple(self.weight.shape)}, expected [{input.shape[1]}]")
        _no_cpu(what, input, target, self.weight)
        if self.bad_targets is None or self.bad_targets.device != input.device:
            self.bad_targets = torch.zeros(1, device=input.device, dtype=torch.int32)
        x = _rows(input)
        t = target.to(torch.int64).contiguous()
        w = None if self.weight is None else self.weight.detach().to(torch.float32).contiguous()
        out = _Criterion.apply(x, t, w, _lib.LOSS_CE, red, int(self.ignore_index), self.bad_targets,
                               x.requires_grad and torch.is_grad_enabled())
        return out.to(input.dtype)
