"""Record what the criterion tests measure, and what the HIP criterion costs, in profiles/loss_errors.json.

"errors": per case of tests/test_loss_gpu.py::test_kernels_against_fp64 (kind, reduction, shape, weighted), the error of
torch's own fp32 criterion on the device and of the HIP modules against torch's fp64 functional on the CPU, in the test's
measure (max |got - ref| / max |ref|).  The test's tolerance is twice the torch figure (floor 4 * 2^-24); the HIP figure is
information, no tolerance is derived from it.

"step": BCE-with-logits (pos_weight, mean) at [8, 23] and [64, 23], criterion forward + backward for both backends: device
launches per call (torch.profiler) and wall time per call, median of three windows of `--iters` calls each after a warm-up
(one synchronize per window).  A record, not a gate: both sides are a few launches on a [B, C] tensor.

    python tools/loss_errors.py [--out profiles/loss_errors.json] [--iters 2000]      # on an MI355X, after build()
"""
import argparse
import json
import os
import re
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import torch  # noqa: E402

import bpmult_amd  # noqa: E402,F401
import test_loss_gpu as T  # noqa: E402


def r4(v):
    return float(f"{v:.4e}")


def short(name):
    """kernel name without its template and argument lists"""
    m = re.search(r"([\w:]+?)\s*[<(]", name.replace("(anonymous namespace)::", "").replace("void ", ""))
    return m.group(1) if m else name


def launches(fn):
    """device kernels of one call, counted by torch.profiler; None (with the reason) where the profiler is unavailable"""
    try:
        from torch.profiler import ProfilerActivity, profile
        fn()
        torch.cuda.synchronize()
        with profile(activities=[ProfilerActivity.CPU, ProfilerActivity.CUDA]) as prof:
            fn()
            torch.cuda.synchronize()
        dev = [e for e in prof.events() if str(getattr(e, "device_type", "")).endswith("CUDA")]
        return len(dev), sorted({short(e.name) for e in dev})
    except Exception as exc:  # noqa: BLE001
        return None, [f"{type(exc).__name__}: {exc}"]


def wall_us(fn, iters):
    for _ in range(200):
        fn()
    torch.cuda.synchronize()
    windows = []
    for _ in range(3):
        t0 = time.perf_counter()
        for _ in range(iters):
            fn()
        torch.cuda.synchronize()
        windows.append((time.perf_counter() - t0) / iters * 1e6)
    return r4(statistics.median(windows)), [r4(w) for w in windows]


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "loss_errors.json"))
    ap.add_argument("--iters", type=int, default=2000)
    a = ap.parse_args()
    out = {"_about": "tools/loss_errors.py; errors: max|got-ref| / max|ref| against torch fp64 on the CPU (loss, grad)",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "errors": {}, "step": {}}
    for kind, red, (B, Cn), weighted in T.CASES:
        d = T.data(kind, B, Cn, weighted)
        e_t = T.torch_f32_errors(kind, d, red)
        got = T.run_module(T.module_for(kind, d.w, red), d.x, d.y)
        e_h = tuple(T.rel_err(g, r) for g, r in zip(got, d.ref[red]))
        out["errors"][f"{kind}-{red}-{B}x{Cn}-{'w' if weighted else 'nw'}"] = {
            "torch_f32": [r4(e) for e in e_t], "hip": [r4(e) for e in e_h], "tolerance": [r4(T.tol_of(e)) for e in e_t]}
    for B in (8, 64):
        g = torch.Generator().manual_seed(B)
        x = torch.randn(B, 23, generator=g).cuda().requires_grad_(True)
        y = (torch.rand(B, 23, generator=g) > 0.5).float().cuda()
        w = (0.5 + 4 * torch.rand(23, generator=g)).cuda()
        rec = {}
        for name, crit in (("torch", T.module_for("bce", w, "mean", hip=False)), ("hip", T.module_for("bce", w, "mean"))):
            def call(crit=crit):
                x.grad = None
                crit(x, y).backward()
            n, names = launches(call)
            med, windows = wall_us(call, a.iters)
            rec[name] = {"launches": n, "kernels": names, "wall_us_per_call": med, "windows_us": windows}
            print(B, name, json.dumps(rec[name]), flush=True)
        out["step"][f"bce-mean-{B}x23-w"] = rec
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
