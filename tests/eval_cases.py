"""Evaluation metrics restated in plain numpy fp64 (no scikit-learn, no torch): the expected values of the evaluation
tests at sizes the fixture f17_eval.npz does not carry.  tests/test_eval_cpu.py checks this file against that fixture,
which the reference's own model_eval and scikit-learn produced (tests/golden/make_golden_eval.py).

Also the table of fixture cases and their deterministic inputs, shared by the generator and the tests.
"""
import numpy as np

from detgen import det

# case -> (task, task_type, N, C, batch size)
CASES = {
    "moviescope": ("moviescope", "multilabel", 300, 13, 64),
    "mmimdb": ("mmimdb", "multilabel", 37, 23, 8),
    "mmimdb_empty": ("mmimdb", "multilabel", 37, 23, 8),          # class 2 has no positive
    "mosei": ("cmu-mosei", "multilabel", 300, 6, 64),
    "counseling": ("counseling", "multilabel", 37, 2, 8),
    "mosi": ("cmu-mosi", "classification", 300, 1, 64),
    "ce": ("iemocap", "classification", 37, 4, 8),
}


def kind_of(task, task_type):
    return "multilabel" if task_type == "multilabel" else "regression" if task == "cmu-mosi" else "classes"


def sigmoid32(x):
    """(float32) sigmoid((float64) x): rounded once."""
    x = np.asarray(x, dtype=np.float64)
    e = np.exp(-np.abs(x))
    return (np.where(x >= 0, 1.0, e) / (1.0 + e)).astype(np.float32)


# torch's CPU sigmoid returns one of two neighbouring floats for these four grid values, depending on whether the element
# falls into the vectorised body or the scalar tail of its loop: where the fixture is generated, equal logits would not
# tie.  They are moved up one grid step; the generator asserts that the reference's score is a function of the logit.
UNSTABLE_GRID = (-5.125, -4.625, -3.75, -1.75)


def grid_logits(name, shape):
    """Logits on a 1/8 grid in [-6, 6]: equal logits tie, distinct ones differ by far more than an fp32 ulp, so a
    ranking of the scores cannot depend on whose sigmoid ran."""
    x = np.clip(np.rint(det(name, shape).astype(np.float64) * 2.5 * 8), -48, 48) / 8
    return np.where(np.isin(x, UNSTABLE_GRID), x + 0.125, x).astype(np.float32)


def regression_ok(x):
    """Grid logits whose predict = sigmoid * 6 - 3 stays more than 1e-3 away from every k + 0.5."""
    p = 6.0 / (1.0 + np.exp(-np.asarray(x, dtype=np.float64))) - 3.0
    return np.abs(p - np.floor(p) - 0.5) > 1e-3


def make_inputs(case):
    """(logits, targets) of a fixture case, by name."""
    task, task_type, N, C, _ = CASES[case]
    kind = kind_of(task, task_type)
    pfx = f"f17.{case}."
    if kind == "multilabel":
        x = grid_logits(pfx + "x", (N, C))
        x[0, 0], x[1, 0], x[2, 0] = 0.0, 1e-9, 1e-6              # predictions 0, 0, 1: the comparison is on the fp32 score
        x[3, 0], x[4, 0] = 20.0, 23.5                            # two different logits that tie at 1.0f
        y = (det(pfx + "y", (N, C)) < -0.5244).astype(np.float32)    # about 30 % positives
        y[:, C - 1] = 0.0
        y[10, C - 1] = 1.0                                       # one class with a single positive
        y[5] = y[6] = 0.0                                        # rows without a positive
        y[3, 0], y[4, 0] = 1.0, 0.0
        if case == "mmimdb_empty":
            y[:, 2] = 0.0
        return x, y
    if kind == "regression":
        grid = np.arange(-48, 49) / 8.0
        grid = grid[regression_ok(grid)]
        idx = np.clip(np.rint((det(pfx + "x", (N,)).astype(np.float64) * 0.25 + 0.5) * (len(grid) - 1)), 0, len(grid) - 1).astype(int)
        x = grid[idx].astype(np.float32)
        y = (np.clip(np.rint(det(pfx + "y", (N,)).astype(np.float64) * 1.5 * 4), -12, 12) / 4).astype(np.float32)
        y[:5] = 0.0                                              # exact zeros: left out of the binary metrics
        return x, y
    x = grid_logits(pfx + "x", (N, C))
    y = (np.abs(det(pfx + "y", (N,))) * 1.7).astype(np.int64) % C
    return x, y


# ----------------------------------------------------------------------------------------------------------------------
def average_precision(y, s):
    """AP = (1 / P) sum over the positives i of TP>=(s_i) / N>=(s_i); 0.0 without a positive.  Equals scikit-learn's
    -sum dR P over distinct thresholds, ties included."""
    y = np.asarray(y).astype(bool).ravel()
    s = np.asarray(s).ravel()
    if not y.any():
        return 0.0
    all_sorted, pos_sorted = np.sort(s), np.sort(s[y])
    q = s[y]
    n_ge = len(all_sorted) - np.searchsorted(all_sorted, q, side="left")
    tp_ge = len(pos_sorted) - np.searchsorted(pos_sorted, q, side="left")
    return float(np.sum(tp_ge.astype(np.float64) / n_ge.astype(np.float64)) / y.sum())


def _f1(tp, fp, fn):
    tp, fp, fn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn))
    den = 2 * tp + fp + fn
    return np.where(den > 0, 2 * tp / np.where(den > 0, den, 1.0), 0.0)


def weighted_acc(tp, fp, fn, tn):
    """train.py:138-163 from counts; NaN where the reference divides by zero."""
    tp, fp, fn, tn = (np.asarray(v, dtype=np.float64) for v in (tp, fp, fn, tn))
    p, n = tp + fn, tn + fp
    ok = (p > 0) & (n > 0)
    wacc = np.where(ok, (tp * n / np.where(ok, p, 1.0) + tn) / np.where(ok, 2 * n, 1.0), np.nan)
    recall, precision = tp / (tp + fn + 1e-8), tp / (tp + fp + 1e-8)
    return wacc, np.where(ok, 2 * recall * precision / (recall + precision + 1e-8), np.nan)


def primitives(kind, logits, targets, losses=None):
    """What metrics.Evaluator.compute() returns, from the whole evaluation's logits and targets."""
    loss = float(np.mean(np.asarray(losses, dtype=np.float64))) if losses is not None and len(losses) else float("nan")
    if kind == "multilabel":
        x, t = np.asarray(logits, dtype=np.float32), np.asarray(targets, dtype=np.float32)
        N, C = x.shape
        s = sigmoid32(x)
        p = s > np.float32(0.5)
        y = t == 1.0
        bad = int(np.sum(~((t == 0.0) | (t == 1.0))))
        tp, fp, fn, tn = ((a & b).sum(0).astype(np.int64) for a, b in ((y, p), (~y, p), (y, ~p), (~y, ~p)))
        f1c = _f1(tp, fp, fn)
        sup = (tp + fn).astype(np.float64)
        ny, npd, both = y.sum(1), p.sum(1), (y & p).sum(1)
        f1s = np.where(ny + npd > 0, 2.0 * both / np.maximum(ny + npd, 1), 0.0)
        apc = np.array([average_precision(y[:, c], s[:, c]) for c in range(C)])
        wacc, wf1 = weighted_acc(tp, fp, fn, tn)
        return {"loss": loss, "bad": bad, "n": N, "tp": tp, "fp": fp, "fn": fn, "tn": tn,
                "f1": {"class": f1c, "macro": float(f1c.mean()), "micro": float(_f1(tp.sum(), fp.sum(), fn.sum())),
                       "weighted": float((f1c * sup).sum() / sup.sum()) if sup.sum() > 0 else 0.0, "samples": float(f1s.mean())},
                "subset_accuracy": float(np.mean((y == p).all(1))),
                "ap": {"class": apc, "macro": float(apc.mean()), "micro": average_precision(y, s),
                       "samples": float(np.mean([average_precision(y[r], s[r]) for r in range(N)]))},
                "wacc": wacc, "wf1": wf1}
    if kind == "regression":
        x, t = np.asarray(logits, dtype=np.float32).reshape(-1), np.asarray(targets, dtype=np.float32)
        predict = (sigmoid32(x) * np.float32(6) - np.float32(3)).astype(np.float32)      # two fp32 roundings, as numpy on float32
        keep = np.ones(len(t), dtype=bool)
        bad = 0
        arg = predict
    else:
        x, t = np.asarray(logits, dtype=np.float32), np.asarray(targets, dtype=np.int64)
        keep = (t >= 0) & (t < x.shape[1])
        bad = int((~keep).sum())
        arg = np.argmax(x, axis=1).astype(np.float32)            # first index on ties
        predict = arg * np.float32(6) - np.float32(3)
    pk, tk, ak = predict[keep].astype(np.float64), t[keep].astype(np.float64), arg[keep].astype(np.float64)
    n = int(keep.sum())
    pc, tc = pk - pk.mean(), tk - tk.mean()
    with np.errstate(divide="ignore", invalid="ignore"):
        corr = float((pc * tc).sum() / np.sqrt((pc * pc).sum() * (tc * tc).sum()))
    nz = tk != 0
    bp, bt = pk[nz] > 0, tk[nz] > 0
    a, b, c, d = (float(v.sum()) for v in (bp & bt, bp & ~bt, ~bp & bt, ~bp & ~bt))
    with np.errstate(divide="ignore", invalid="ignore"):
        # f1_score(binary_preds, binary_truth, average='weighted'): the supports are those of the PREDICTIONS
        wf = float(((a + b) * _f1(a, b, c) + (c + d) * _f1(d, c, b)) / np.float64(a + b + c + d))
        acc2 = float(np.float64(a + d) / np.float64(a + b + c + d))
    return {"loss": loss, "bad": bad, "n": n, "mae": float(np.abs(pk - tk).mean()), "corr": corr,
            "accuracy_7": float(np.sum(np.round(pk) == np.round(tk)) / n), "accuracy_2": acc2, "weighted_f1": wf,
            "acc": float(np.mean(ak == tk))}


def reference_metrics(task, task_type, logits, targets, losses):
    """The dict of the reference's model_eval (train.py:195-270), its mislabelled keys included."""
    m = primitives(kind_of(task, task_type), logits, targets, losses)
    out = {"loss": m["loss"]}
    if task_type != "multilabel":
        out.update(mae=m["mae"], corr=m["corr"], accuracy_7=m["accuracy_7"], weighted_f1=m["weighted_f1"], weight_f1=m["mae"])
        return out
    f1, ap = m["f1"], m["ap"]
    if task == "moviescope":
        out.update(macro_f1=f1["macro"], micro_f1=f1["micro"], auc_pr_macro=ap["macro"], auc_pr_micro=ap["micro"], auc_pr_samples=ap["samples"])
    elif task == "mmimdb":
        out.update(macro_f1=f1["macro"], micro_f1=ap["micro"], auc_pr_macro=f1["weighted"], auc_pr_micro=f1["micro"], auc_pr_samples=f1["samples"])
    elif task == "counseling":
        out.update(f1_low=m["wf1"][1], f1_high=m["wf1"][0], acc=m["subset_accuracy"], auc_pr_micro=ap["micro"])
    else:
        C = len(m["wf1"])
        for i in range(C):
            out[f"f1_emo{i + 1}"], out[f"wacc_emo{i + 1}"] = m["wf1"][i], m["wacc"][i]
        out.update(f1_emos=np.mean(m["wf1"]), wacc_emos=ap["micro"], auc_pr_micro=np.mean(m["wacc"]))
    return {k: float(v) for k, v in out.items()}


def batches_of(n, bs):
    return [(i, min(i + bs, n)) for i in range(0, n, bs)]
