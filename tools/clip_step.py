#!/usr/bin/env python3
"""Cost of global-norm gradient clipping in the optimizer phase of a bench.py configuration (one GPU), three ways on the
same model and the same gradients, HIP events around each phase, the variants alternating in one process:

  a  FusedAdam.step()                                                      (no clipping)
  b  torch.nn.utils.clip_grad_norm_(model.parameters(), c); FusedAdam.step()
  c  FusedAdam(max_grad_norm=c).step()                                      (bpm_grad_sumsq + bpm_adam_step_groups)

and the reduction alone (ParamStore.grad_sumsq: both launches), with the HBM rate it reaches over the bytes it reads.

  python tools/clip_step.py [--config h768 --reps 7 --precision bf16]

Prints one JSON line (medians, ms)."""
import argparse
import json
import os
import statistics
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CONFIGS, make_model, run_model, synth_batch  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="h768", choices=sorted(CONFIGS))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "bf16x3", "f32"))
    ap.add_argument("--max-norm", type=float, default=0.8)
    a = ap.parse_args()
    import bpmult_amd  # noqa: F401
    from bpmult_amd.optim import FusedAdam

    c = CONFIGS[a.config]
    torch.manual_seed(1234)
    model = make_model(c, a.precision).to("cuda").train()
    batch = synth_batch(c, c["batch"], 1234, "cuda")
    crit = torch.nn.BCEWithLogitsLoss()
    for _ in range(2):                                      # real gradients in the flat buffer and on the tail
        for p in model.parameters():
            p.grad = None
        crit(run_model(model, batch), batch["tgt"]).backward()
    st = model._store
    plain = FusedAdam(model, lr=1e-5)
    fused = FusedAdam(model, lr=1e-5, max_grad_norm=a.max_norm)
    params = list(model.parameters())

    def var_a():
        plain.step()

    def var_b():
        torch.nn.utils.clip_grad_norm_(params, a.max_norm)
        plain.step()

    def var_c():
        fused.step()

    def reduction():
        st.grad_sumsq(1.0, a.max_norm)

    variants = {"a_adam": var_a, "b_torch_clip_adam": var_b, "c_fused_clip_adam": var_c, "reduction": reduction}
    for f in variants.values():                             # moments, tables, workspaces: allocated outside the timing
        f()
        f()
    torch.cuda.synchronize()
    ms = {k: [] for k in variants}
    for _ in range(a.reps):
        for k, f in variants.items():
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            f()
            e1.record()
            e1.synchronize()
            ms[k].append(e0.elapsed_time(e1))
    med = {k: round(statistics.median(v), 4) for k, v in ms.items()}
    nbytes = 4 * sum(p.numel() for p in st.params.values() if p.requires_grad)
    out = {"config": a.config, "precision": a.precision, "reps": a.reps, "max_norm": a.max_norm, "median_ms": med,
           "min_ms": {k: round(min(v), 4) for k, v in ms.items()},
           "trunk_grad_bytes": nbytes, "flat_buffer_bytes": 4 * st.total, "norm_segments": st._norm_table[1],
           "norm_blocks": st._norm_table[2], "reduction_TBps": round(nbytes / (med["reduction"] * 1e-3) / 1e12, 3),
           "clip_cost_ms": {"torch": round(med["b_torch_clip_adam"] - med["a_adam"], 4),
                            "fused": round(med["c_fused_clip_adam"] - med["a_adam"], 4)},
           "last_grad_norm": float(fused.last_grad_norm)}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
