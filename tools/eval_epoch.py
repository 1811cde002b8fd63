"""Time an evaluation epoch of the headline model both ways, and record the evaluation tests' measured errors.

profiles/eval_epoch.json: the headline model (bench.py config h768 with 23 classes, bf16, eval mode), B = 8, 64 batches,
after a warm-up.  Two loops alternate in one process, each repeated `--repeats` times, host clock around a final
synchronise:
  (a) "reference": the loop as the reference writes it (train.py:165-280) -- per batch loss.item() and .cpu() copies of
      the sigmoid, the prediction and the target -- with the metrics from the numpy restatement (tests/eval_cases.py) on the
      host;
  (b) "evaluator": training.model_eval's loop over metrics.Evaluator -- one launch per batch, one read at the end.
Both run the same forward and the same criterion on the same batches.  Also the finalize alone at N = 8192, C = 23
(device events around the launches, median of `--repeats`).  A record, not a gate.

profiles/eval_errors.json (--errors): per fixture case of tests/test_eval_gpu.py, the largest |metric - fixture| of
Evaluator / model_eval against tests/golden/f17_eval.npz, and of the primitives against the numpy restatement.

    python tools/eval_epoch.py [--errors] [--repeats 5]      # on an MI355X, after build()
"""
import argparse
import json
import os
import statistics
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests"), os.path.join(ROOT, "tests", "golden")):
    if p not in sys.path:
        sys.path.insert(0, p)

import numpy as np  # noqa: E402
import torch  # noqa: E402

import bench  # noqa: E402
import bpmult_amd  # noqa: E402,F401
import eval_cases as ec  # noqa: E402
from bpmult_amd import metrics, ops, training  # noqa: E402

B, NBATCH, CLASSES = 8, 64, 23


def r4(v):
    return float(f"{v:.4e}")


def errors(out_path):
    import test_eval_gpu as T
    rec = {"_about": "tools/eval_epoch.py --errors; max |metric - fixture| against tests/golden/f17_eval.npz (mae / corr / weight_f1 "
                     "relative: the reference computes them in float32) and max |primitive - numpy restatement|",
           "device": torch.cuda.get_device_name(0), "tolerance": {"fp64": T.TOL, "float32_reference_relative": 1e-5}, "cases": {}}
    for case, (a, b, prim) in T.fixture_errors().items():
        task, task_type, N, Cn, bs = ec.CASES[case]
        kind = ec.kind_of(task, task_type)
        want = T.fixture_metrics(case)
        f32 = [k for k in want if k in T.F32_KEYS and kind != "multilabel"]
        exp = ec.primitives(kind, T.FIX[case + ".logits"], T.FIX[case + ".targets"], T.FIX[case + ".losses"])
        rec["cases"][case] = {
            "evaluator_fp64": r4(max(abs(a[k] - w) for k, w in want.items() if k not in f32)),
            "model_eval_fp64": r4(max(abs(b[k] - w) for k, w in want.items() if k not in f32)),
            "float32_reference_relative": r4(max((abs(a[k] - want[k]) / abs(want[k]) for k in f32), default=0.0)),
            "primitives_against_restatement": r4(T.max_err(prim, exp))}
        print(case, json.dumps(rec["cases"][case]), flush=True)
    with open(out_path, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", out_path)


def reference_loop(model, crit, batches):
    """model_eval as the reference writes it: four host syncs per batch, metrics on the host."""
    losses, preds, tgts, raw = [], [], [], []
    with torch.no_grad():
        for b in batches:
            out = bench.run_model(model, b)
            loss = crit(out, b["tgt"])
            losses.append(loss.item())
            preds.append(torch.sigmoid(out).cpu().detach().numpy() > 0.5)
            raw.append(torch.sigmoid(out).cpu().detach().numpy())
            tgts.append(b["tgt"].cpu().detach().numpy())
    x = np.vstack(raw)
    # the restatement takes logits; hand it the scores' logits so that the host work is the same O(n log n) ranking
    with np.errstate(divide="ignore"):
        logits = np.log(x / (1 - x))
    return ec.primitives("multilabel", logits, np.vstack(tgts), losses)["ap"]["micro"]


def evaluator_loop(model, crit, batches, ev):
    ev.reset()
    with torch.no_grad():
        for b in batches:
            out = bench.run_model(model, b)
            ev.update(out, b["tgt"], crit(out, b["tgt"]))
    return ev.compute()["ap"]["micro"]


def timed(fn):
    torch.cuda.synchronize()
    t0 = time.perf_counter()
    fn()
    torch.cuda.synchronize()
    return (time.perf_counter() - t0) * 1e3


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_epoch.json"))
    ap.add_argument("--errors", action="store_true", help="also write profiles/eval_errors.json")
    ap.add_argument("--repeats", type=int, default=5)
    a = ap.parse_args()
    dev = torch.device("cuda")
    if a.errors:
        errors(os.path.join(os.path.dirname(os.path.abspath(a.out)), "eval_errors.json"))
    c = dict(bench.CONFIGS["h768"], n_classes=CLASSES)
    torch.manual_seed(0)
    model = bench.make_model(c, "bf16", dropout=False).to(dev).eval()
    batches = [bench.synth_batch(c, B, 1000 + i, dev) for i in range(NBATCH)]
    from bpmult_amd import losses
    crit = losses.BCEWithLogitsLoss()
    ev = metrics.Evaluator("multilabel", CLASSES, B * NBATCH, NBATCH, device=dev)
    loops = {"reference": lambda: reference_loop(model, crit, batches), "evaluator": lambda: evaluator_loop(model, crit, batches, ev)}
    for fn in loops.values():           # warm-up: graph capture, allocator
        fn()
        fn()
    times = {k: [] for k in loops}
    for _ in range(a.repeats):          # alternate, so that drift hits both
        for k, fn in loops.items():
            times[k].append(timed(fn))
    rec = {"_about": "tools/eval_epoch.py; ms per evaluation epoch (64 batches of 8, 23 classes, h768 bf16 eval mode), host clock "
                     "around a final synchronise, the two loops alternating",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__, "epoch_ms": {}}
    for k, v in times.items():
        rec["epoch_ms"][k] = {"median": r4(statistics.median(v)), "min": r4(min(v)), "max": r4(max(v)), "runs": [r4(t) for t in v]}
        print(k, json.dumps(rec["epoch_ms"][k]), flush=True)
    # the finalize alone at MM-IMDb's size
    N = 8192
    rng = np.random.default_rng(0)
    big = metrics.Evaluator("multilabel", CLASSES, N, 8, device=dev)
    x = torch.from_numpy(rng.standard_normal((N, CLASSES)).astype(np.float32)).to(dev)
    y = torch.from_numpy((rng.random((N, CLASSES)) < 0.1).astype(np.float32)).to(dev)
    for i in range(0, N, 1024):
        big.update(x[i:i + 1024], y[i:i + 1024])
    fin = []
    for _ in range(a.repeats + 1):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        ops.eval_finalize(big._desc, big.n, 0)
        e1.record()
        torch.cuda.synchronize()
        fin.append(e0.elapsed_time(e1))
    fin = fin[1:]
    rec["finalize_ms_8192x23"] = {"median": r4(statistics.median(fin)), "min": r4(min(fin)), "max": r4(max(fin))}
    print("finalize", json.dumps(rec["finalize_ms_8192x23"]), flush=True)
    os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print("wrote", a.out)


if __name__ == "__main__":
    main()
