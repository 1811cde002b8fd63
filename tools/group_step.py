#!/usr/bin/env python3
"""Cost of parameter groups, decoupled decay and the non-finite skip in the optimizer phase of a bench.py configuration
(one GPU), four ways on the same model and the same gradients, HIP events around each step, the variants alternating in
one process after warm-up.  Every variant is the same launch, bpm_adam_step_groups, over a table of its own:

  a  FusedAdam(model)                                               (one L2 group over the whole trunk)
  b  FusedAdam(param_groups=decay_groups(decoupled_weight_decay))   (two groups)
  c  b with skip_nonfinite=True                                     (+ bpm_grad_sumsq, device counters, fused torch Adam on the tail)
  d  b with one large matrix left out of every group                (a segment that is not stepped)

`a` is timed twice per round (a_adam, a_adam_again): the distance between the two medians and their min..max ranges are
the spread the others are to be read against.

  python tools/group_step.py [--config h768 --reps 9 --precision bf16]

Prints one JSON line (ms)."""
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
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "bf16x3", "f32"))
    a = ap.parse_args()
    import bpmult_amd  # noqa: F401
    from bpmult_amd.optim import FusedAdam, decay_groups

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
    groups = decay_groups(model, 0.01, decoupled_weight_decay=True)
    big = max((p for n, p in st.params.items() if n in st._adam_plain), key=lambda p: p.numel())
    without = [dict(g, params=[p for p in g["params"] if p is not big]) for g in groups]
    opts = {"a_adam": FusedAdam(model, lr=1e-5),
            "b_groups_decoupled": FusedAdam(model, lr=1e-5, param_groups=groups),
            "c_groups_skip_nonfinite": FusedAdam(model, lr=1e-5, param_groups=groups, skip_nonfinite=True),
            "d_groups_one_matrix_out": FusedAdam(model, lr=1e-5, param_groups=without)}
    variants = {k: o.step for k, o in opts.items()}
    variants["a_adam_again"] = opts["a_adam"].step
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
    out = {"config": a.config, "precision": a.precision, "reps": a.reps, "median_ms": med,
           "min_ms": {k: round(min(v), 4) for k, v in ms.items()}, "max_ms": {k: round(max(v), 4) for k, v in ms.items()},
           "flat_buffer_bytes": 4 * st.total, "left_out_elements": big.numel(),
           "segments_blocks": {k: o._group_table[1:] for k, o in opts.items()}, "skipped_steps": int(opts["c_groups_skip_nonfinite"].skipped_steps),
           "vs_a_ms": {k: round(med[k] - med["a_adam"], 4) for k in med if k != "a_adam"}}
    print(json.dumps(out))


if __name__ == "__main__":
    main()
