#!/usr/bin/env python3
"""Whole training step (zero-grad, forward, BCE loss, backward; one GPU) of a bench.py configuration at a chosen number of
heads: the same model, batch and timing as `bench.py --config NAME` with `num_heads` replaced (head_dim = hidden / heads).

  python tools/model_step.py --config cfg5 --heads 6 12 [--steps 10 --warmup 4 --precision bf16]

Prints one JSON line: ms per step for each head count, measured one after the other in this process (host clock around
`--steps` steps that end in a device synchronise, after `--warmup` untimed steps: the step is captured into hipGraphs
on its 3rd / 4th call)."""
import argparse
import json
import os
import sys
import time

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
from bench import CONFIGS, make_model, run_model, synth_batch  # noqa: E402


def step_ms(c, precision, steps, warmup, dev):
    torch.manual_seed(1234)
    model = make_model(c, precision).to(dev).train()
    batch = synth_batch(c, c["batch"], 1234, dev)
    crit = torch.nn.BCEWithLogitsLoss()

    def step():
        for p in model.parameters():
            p.grad = None
        loss = crit(run_model(model, batch), batch["tgt"])
        loss.backward()
        return loss

    for _ in range(max(warmup, 4)):
        step()
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    for _ in range(steps):
        loss = step()
    torch.cuda.synchronize()
    ms = (time.perf_counter() - t0) / steps * 1e3
    out = {"ms_per_step": round(ms, 2), "loss": round(float(loss.detach()), 5)}
    del model, batch
    torch.cuda.empty_cache()
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--config", default="cfg5", choices=sorted(CONFIGS))
    ap.add_argument("--heads", type=int, nargs="+", required=True)
    ap.add_argument("--steps", type=int, default=10)
    ap.add_argument("--warmup", type=int, default=4)
    ap.add_argument("--precision", default="bf16", choices=("bf16", "bf16x3", "f32"))
    a = ap.parse_args()
    import bpmult_amd  # noqa: F401
    base = CONFIGS[a.config]
    res = {"config": a.config, "hidden": base["hidden_sz"], "precision": a.precision, "batch": base["batch"], "steps": a.steps}
    for H in a.heads:
        if base["hidden_sz"] % H:
            raise SystemExit(f"hidden {base['hidden_sz']} is not divisible by {H} heads")
        c = dict(base, num_heads=H)
        res[f"heads{H}"] = dict(head_dim=base["hidden_sz"] // H, **step_ms(c, a.precision, a.steps, a.warmup, "cuda"))
    print(json.dumps(res))


if __name__ == "__main__":
    main()
