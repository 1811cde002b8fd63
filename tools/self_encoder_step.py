#!/usr/bin/env python3
"""Forward + backward of a standalone TransformerEncoder on one GPU: the self-attention stack forward(x) beside the
crossmodal stack forward(x, x_kv, x_kv) at the same shape (S = T), eager launches as the module runs them.

  python tools/self_encoder_step.py [--steps 20 --warmup 5 --precision bf16]

Shapes: d=768 / 12 heads / 5 layers / T=512 / B=8, and the kernel point's d=768 / 6 heads / 5 layers / T=50 / B=64.
Timing as in tools/model_step.py: `--warmup` untimed steps, then `--steps` steps between two device synchronisations,
timed with events on the current stream.  Flops (algorithmic, the formula of tools/kernel_point.py plus the FFN), per
sample and layer:  (4 T + 4 S) d^2 + 4 pairs d  (projections + attention; pairs = T (T + 1) / 2 with the causal mask)
+ 16 T d^2 (fc1, fc2); forward + backward = 3x.  Prints one JSON line: ms per step, TFLOP/s and the fraction of the bf16
MFMA peak (bench.PEAK_BF16_TFLOPS)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import PEAK_BF16_TFLOPS, PEAK_F32_TFLOPS  # noqa: E402

SHAPES = {"t512": dict(d=768, H=12, L=5, T=512, B=8), "kernel_point": dict(d=768, H=6, L=5, T=50, B=64)}


def flops(d, L, T, B, mask=True):
    S = T
    pairs = T * (T + 1) // 2 if mask else T * S
    return 3 * B * L * ((4 * T + 4 * S) * d * d + 4 * pairs * d + 16 * T * d * d)


def step_ms(sh, cross, precision, steps, warmup):
    from bpmult_amd.models.encoder import TransformerEncoder
    torch.manual_seed(1234)
    enc = TransformerEncoder(sh["d"], sh["H"], sh["L"], attn_mask=True)
    enc.precision = precision
    enc = enc.cuda().train()
    x = torch.randn(sh["T"], sh["B"], sh["d"], device="cuda", requires_grad=True)
    kv = torch.randn(sh["T"], sh["B"], sh["d"], device="cuda", requires_grad=True) if cross else None
    w = torch.randn(sh["T"], sh["B"], sh["d"], device="cuda")

    def step():
        for p in enc.parameters():
            p.grad = None
        x.grad = None
        y = enc(x, kv, kv) if cross else enc(x)
        (y * w).sum().backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
    e0.record()
    for _ in range(steps):
        step()
    e1.record()
    torch.cuda.synchronize()
    ms = e0.elapsed_time(e1) / steps
    del enc, x, kv, w
    torch.cuda.empty_cache()
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "bf16x3", "f32"))
    a = ap.parse_args()
    import bpmult_amd  # noqa: F401
    peak = PEAK_F32_TFLOPS if a.precision == "f32" else PEAK_BF16_TFLOPS
    res = {"precision": a.precision, "steps": a.steps, "warmup": a.warmup, "peak_tflops": peak}
    for name, sh in SHAPES.items():
        fl = flops(sh["d"], sh["L"], sh["T"], sh["B"])
        out = dict(sh, gflop_per_step=round(fl / 1e9, 1))
        for kind, cross in (("self", False), ("crossmodal", True)):
            ms = step_ms(sh, cross, a.precision, a.steps, a.warmup)
            tf = fl / (ms * 1e-3) / 1e12
            out[kind] = {"ms_per_step": round(ms, 3), "tflops": round(tf, 1), "frac_peak": round(tf / peak, 4)}
        res[name] = out
    print(json.dumps(res))


if __name__ == "__main__":
    main()
