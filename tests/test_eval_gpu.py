"""Evaluation on the HIP path (csrc/eval.hip, metrics.Evaluator, training.model_eval) on the device.

Fixture parity: every case of tests/golden/f17_eval.npz -- the dict of the reference's own model_eval with scikit-learn --
through Evaluator and through model_eval.  Integer counts are exact; the fp64 metrics are held to 1e-9 (a fixed-order fp64
sum of n terms in [0, 1] carries at most n 2^-53 = 1.2e-10 at n = N C = 2^20, far above the sizes here); mae / corr to
1e-5 relative, because the REFERENCE computes them from float32 numpy arrays (pairwise float32 summation over 300 terms
plus the two fp32 roundings of predict: about 1e-6).  Everywhere else the expected values are the numpy fp64 restatement
of tests/eval_cases.py (checked against the fixture by tests/test_eval_cpu.py), to 1e-9.

Kernel geometry the shapes are chosen around: 256 query elements per block, LDS chunks of 1024 keys, list splits of 8192
keys, 1024 elements per block of the quotient / row sums, 256 rows per block of the per-row kernel."""
import os
import warnings
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

import eval_cases as ec  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import losses, metrics, ops, training  # noqa: E402

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FIX = np.load(os.path.join(ROOT, "tests", "golden", "f17_eval.npz"))
DEV = "cuda"
TOL = 1e-9
F32_KEYS = ("mae", "corr", "weight_f1")
T = torch.from_numpy


def fixture_metrics(case):
    pfx = case + ".m."
    return {k[len(pfx):]: float(FIX[k]) for k in FIX.files if k.startswith(pfx)}


def evaluate(kind, x, y, bs, losses_=None, pad=0, capacity=None, ev=None):
    """The whole evaluation through Evaluator in batches of bs; pad: extra columns of the logits / targets buffers."""
    N = len(x)
    Cn = 1 if kind == "regression" else x.shape[1]
    spans = ec.batches_of(N, bs)
    if ev is None:
        ev = metrics.Evaluator(kind, Cn, capacity or N, max_batches=len(spans), device=DEV)
    for i, (lo, hi) in enumerate(spans):
        xb, yb = T(np.ascontiguousarray(x[lo:hi])).to(DEV), T(np.ascontiguousarray(y[lo:hi])).to(DEV)
        if pad:
            buf = torch.full((hi - lo, Cn + pad), float("nan"), device=DEV)
            buf[:, :Cn] = xb.reshape(hi - lo, Cn)
            xb = buf[:, :Cn]
            if kind == "multilabel":
                tb = torch.full((hi - lo, Cn + pad), 7.0, device=DEV)
                tb[:, :Cn] = yb
                yb = tb[:, :Cn]
        ev.update(xb, yb, None if losses_ is None else torch.tensor(losses_[i], dtype=torch.float32, device=DEV))
    return ev, ev.compute()


def assert_same(got, want, tol=TOL, path=""):
    """Integers (and integer arrays) exact, floats within tol, NaN where NaN."""
    assert set(got) == set(want), (path, set(got) ^ set(want))
    for k, w in want.items():
        g = got[k]
        if isinstance(w, dict):
            assert_same(g, w, tol, path + k + ".")
        elif isinstance(w, (int, np.integer)) or (isinstance(w, np.ndarray) and w.dtype.kind in "iu"):
            assert np.array_equal(np.asarray(g), np.asarray(w)), (path + k, g, w)
        else:
            g, w = np.asarray(g, dtype=np.float64), np.asarray(w, dtype=np.float64)
            assert g.shape == w.shape and np.array_equal(np.isnan(g), np.isnan(w)), (path + k, g, w)
            assert np.all(np.abs(g - w)[~np.isnan(w)] <= tol), (path + k, g, w)


def max_err(got, want):
    worst = 0.0
    for k, w in want.items():
        if isinstance(w, dict):
            worst = max(worst, max_err(got[k], w))
        else:
            d = np.abs(np.asarray(got[k], dtype=np.float64) - np.asarray(w, dtype=np.float64))
            worst = max(worst, float(np.nanmax(d)) if d.size else 0.0)
    return worst


def random_case(kind, N, Cn, seed):
    """Grid logits (many exact ties) and about 30 % positives / uniform classes / quarter-grid targets."""
    rng = np.random.default_rng(seed)
    if kind == "multilabel":
        return (rng.integers(-24, 25, (N, Cn)) / 8).astype(np.float32), (rng.random((N, Cn)) < 0.3).astype(np.float32)
    if kind == "regression":
        return (rng.integers(-24, 25, N) / 8).astype(np.float32), (rng.integers(-12, 13, N) / 4).astype(np.float32)
    return (rng.integers(-24, 25, (N, Cn)) / 8).astype(np.float32), rng.integers(0, Cn, N).astype(np.int64)


class Handout(torch.nn.Module):
    """A model that returns the logits it is handed in the batch's image slot (what the fixture generator does to the
    reference's model_forward)."""

    def __init__(self):
        super().__init__()
        self.p = torch.nn.Parameter(torch.zeros(1))

    def forward(self, txt, mask, segment, img, audio):
        return img


def handout_batches(x, y, bs):
    z = torch.zeros(1, 1, dtype=torch.long)
    return [(torch.zeros(hi - lo, 1, dtype=torch.long), z, z, T(np.ascontiguousarray(x[lo:hi])), T(np.ascontiguousarray(y[lo:hi])), z)
            for lo, hi in ec.batches_of(len(x), bs)]


def fixture_errors():
    """Per fixture case, the largest |metric - fixture| of Evaluator and of model_eval (tools/eval_epoch.py records it)."""
    out = {}
    for case, (task, task_type, N, Cn, bs) in ec.CASES.items():
        x, y, ls = FIX[case + ".logits"], FIX[case + ".targets"], FIX[case + ".losses"]
        kind = ec.kind_of(task, task_type)
        args = SimpleNamespace(task=task, task_type=task_type, model="mmtrvat", n_classes=Cn)
        _, prim = evaluate(kind, x, y, bs, ls)
        a = training.arrange_metrics(args, prim)
        it = iter(ls)
        crit = lambda out, tgt: torch.tensor(next(it), dtype=torch.float32, device=DEV)      # noqa: E731
        xm = x.reshape(N, 1) if kind == "regression" else x
        b = training.model_eval(Handout().to(DEV), crit, handout_batches(xm, y, bs), args)
        out[case] = (a, b, prim)
    return out


@pytest.fixture(scope="module")
def fixture_runs():
    return fixture_errors()


@pytest.mark.parametrize("case", list(ec.CASES))
def test_fixture_parity(case, fixture_runs):
    task, task_type, N, Cn, bs = ec.CASES[case]
    kind = ec.kind_of(task, task_type)
    want = fixture_metrics(case)
    via_evaluator, via_model_eval, prim = fixture_runs[case]
    for name, got in (("Evaluator", via_evaluator), ("model_eval", via_model_eval)):
        assert set(got) == set(want) | ({"acc"} if kind == "classes" else set())
        for k, w in want.items():
            err = abs(got[k] - w)
            print(f"{case} {name} {k}: {got[k]!r} against {w!r}, error {err:.3e}")
            # the batch losses are fp32 values: their fp64 mean is exact to rounding
            assert err <= (1e-5 * abs(w) if k in F32_KEYS and kind != "multilabel" else TOL), (name, k, got[k], w)
    assert via_evaluator == via_model_eval
    # integer counts and accuracy_7 against the restatement: exact
    exp = ec.primitives(kind, FIX[case + ".logits"], FIX[case + ".targets"], FIX[case + ".losses"])
    assert prim["bad"] == 0 and prim["n"] == N
    if kind == "multilabel":
        for k in ("tp", "fp", "fn", "tn"):
            assert np.array_equal(prim[k], exp[k]), k
        assert prim["subset_accuracy"] == exp["subset_accuracy"]
    else:
        assert prim["accuracy_7"] == want["accuracy_7"] and prim["accuracy_2"] == exp["accuracy_2"]
    assert_same(prim, exp)


SHAPES = [(1, 1), (37, 5), (300, 23), (255, 3), (256, 4), (257, 1), (1023, 1), (1024, 1), (1025, 1), (1024, 8), (8191, 1),
          (8192, 1), (8193, 1)]


@pytest.mark.parametrize("N,Cn", SHAPES)
def test_multilabel_shapes(N, Cn):
    x, y = random_case("multilabel", N, Cn, 100 * N + Cn)
    bs = 8 if N <= 64 else 1000
    ls = [0.25 * (i + 1) for i in range(len(ec.batches_of(N, bs)))]
    _, got = evaluate("multilabel", x, y, bs, ls)                 # capacity filled exactly
    assert_same(got, ec.primitives("multilabel", x, y, ls))


@pytest.mark.parametrize("kind", ["regression", "classes"])
@pytest.mark.parametrize("N", [1, 37, 1023, 1024, 1025, 2500])
def test_row_kind_shapes(kind, N):
    x, y = random_case(kind, N, 4, N)
    ls = [1.5, 0.5] if N > 8 else [1.5]
    _, got = evaluate(kind, x, y, (N + 1) // 2 if N > 8 else 8, ls)
    assert_same(got, ec.primitives(kind, x, y, ls))


def test_padded_rows_spare_capacity_and_no_losses():
    x, y = random_case("multilabel", 37, 5, 1)
    exp = ec.primitives("multilabel", x, y)
    ev, got = evaluate("multilabel", x, y, 8, pad=3, capacity=64)     # batches 8, 8, 8, 8, 5 out of buffers [B, 8]
    assert ev.nbatches == 5 and np.isnan(got["loss"])
    assert_same(got, exp)
    xr, yr = random_case("regression", 37, 1, 2)
    _, got = evaluate("regression", xr.reshape(-1, 1), yr, 8, pad=2)   # logits [B, 1] with a row stride of 3
    assert_same(got, ec.primitives("regression", xr, yr))
    xc, yc = random_case("classes", 37, 4, 3)
    _, got = evaluate("classes", xc, yc, 8, pad=4)
    assert_same(got, ec.primitives("classes", xc, yc))


def test_ties_and_one_sided_classes():
    N, Cn = 300, 4
    x, y = random_case("multilabel", N, Cn, 5)
    x[:] = 0.375                                                  # every score tied: AP of a list = its share of positives
    y[:, 1], y[:, 2] = 0.0, 1.0                                   # a class without a positive, a class without a negative
    _, got = evaluate("multilabel", x, y, 64)
    assert_same(got, ec.primitives("multilabel", x, y))
    assert got["ap"]["class"][1] == 0.0 and got["ap"]["class"][2] == 1.0
    assert abs(got["ap"]["class"][0] - y[:, 0].mean(dtype=np.float64)) <= 1e-12 and abs(got["ap"]["micro"] - y.mean(dtype=np.float64)) <= 1e-12
    assert np.isnan(got["wacc"][1]) and np.isnan(got["wacc"][2]) and np.isnan(got["wf1"][1])
    x2, y2 = random_case("multilabel", N, Cn, 6)
    x2[:, 3] = 23.5                                               # saturated scores: all 1.0f
    _, got = evaluate("multilabel", x2, y2, 64)
    assert_same(got, ec.primitives("multilabel", x2, y2))


def test_prediction_is_compared_on_the_fp32_score():
    x = np.array([[0.0, 1e-9, 1e-6, -1e-6, 20.0, 23.5]], dtype=np.float32)
    y = np.array([[1, 1, 1, 0, 1, 0]], dtype=np.float32)
    ev, got = evaluate("multilabel", x, y, 1)
    tgt, pred, score = ev.predictions()
    assert pred.tolist() == [[False, False, True, False, True, True]]
    assert score[0, 0] == score[0, 1] == np.float32(0.5) and score[0, 4] == score[0, 5] == np.float32(1.0)
    assert np.array_equal(score, ec.sigmoid32(x)) and np.array_equal(tgt, y)
    xr = np.array([0.0, 0.625, -2.5, 5.0], dtype=np.float32)
    ev, _ = evaluate("regression", xr, np.zeros(4, dtype=np.float32), 4)
    tgt, pred, raw = ev.predictions()
    assert np.array_equal(pred, ec.sigmoid32(xr)) and np.array_equal(raw, xr)
    # predict = pred * 6 - 3 in two fp32 roundings (no fused multiply-add)
    want = (ec.sigmoid32(xr) * np.float32(6)).astype(np.float32) - np.float32(3)
    assert np.array_equal(ev._predict[:4].cpu().numpy(), want)


def test_two_runs_give_identical_bits_and_reset_repeats():
    x, y = random_case("multilabel", 300, 23, 9)
    ls = [0.1, 0.2, 0.3, 0.4, 0.7]
    ev, a = evaluate("multilabel", x, y, 64, ls)
    raw_a = ev._out.cpu().numpy().copy()
    ev.reset()
    assert ev.n == 0 and ev.nbatches == 0
    _, b = evaluate("multilabel", x, y, 64, ls, ev=ev)
    assert np.array_equal(raw_a, ev._out.cpu().numpy())
    _, c = evaluate("multilabel", x, y, 64, ls)                   # a fresh store, other batch boundaries below
    assert_same(b, a, tol=0.0)
    assert_same(c, a, tol=0.0)
    _, d = evaluate("multilabel", x, y, 300, None)
    d["loss"] = a["loss"]
    assert_same(d, a, tol=0.0)                                    # the metrics do not depend on how the rows arrived
    for kind in ("regression", "classes"):
        xr, yr = random_case(kind, 2500, 4, 10)
        ev, a = evaluate(kind, xr, yr, 1000)
        ev.reset()
        _, b = evaluate(kind, xr, yr, 1000, ev=ev)
        assert_same(b, a, tol=0.0)


def test_update_does_not_synchronise_and_compute_does_once():
    x, y = random_case("multilabel", 24, 5, 11)
    ev = metrics.Evaluator("multilabel", 5, 24, device=DEV)
    xs = [T(x[i:i + 8]).to(DEV) for i in (0, 8, 16)]
    ys = [T(y[i:i + 8]).to(DEV) for i in (0, 8, 16)]
    ls = [torch.tensor(float(i), device=DEV) for i in range(3)]
    gates = torch.ones(8, 12, device=DEV)
    torch.cuda.synchronize()
    prev = torch.cuda.get_sync_debug_mode()
    try:
        torch.cuda.set_sync_debug_mode("error")
        for xb, yb, lb in zip(xs, ys, ls):
            ev.update(xb, yb, lb, gates)
        ops.eval_finalize(ev._desc, ev.n, ev.nlosses)             # the finalize launches do not synchronise either
        with pytest.raises(RuntimeError, match="synchroniz"):
            ev.compute()
        torch.cuda.set_sync_debug_mode("warn")
        with warnings.catch_warnings(record=True) as rec:
            warnings.simplefilter("always")
            got = ev.compute()
        assert len([w for w in rec if "synchroniz" in str(w.message)]) == 1, [str(w.message) for w in rec]
    finally:
        torch.cuda.set_sync_debug_mode(prev)
    assert_same(got, ec.primitives("multilabel", x, y, [0.0, 1.0, 2.0]))
    assert ev.predictions()[3].shape == (24, 12)


def test_refused_targets_are_counted():
    x, y = random_case("multilabel", 37, 5, 12)
    y[0, 0], y[3, 2], y[36, 4] = 0.5, 2.0, np.nan                 # stored as label 0
    ev, got = evaluate("multilabel", x, y, 8)
    assert got["bad"] == 3
    y0 = y.copy()
    y0[0, 0] = y0[3, 2] = y0[36, 4] = 0.0
    exp = ec.primitives("multilabel", x, y0)
    exp["bad"] = 3
    assert_same(got, exp)
    ev.reset()
    _, again = evaluate("multilabel", x, y0, 8, ev=ev)
    assert again["bad"] == 0                                      # reset clears the counter
    xc, yc = random_case("classes", 37, 4, 13)
    yc[1], yc[20], yc[36] = -1, 4, 1 << 40                        # rows excluded from every count and sum
    _, got = evaluate("classes", xc, yc, 8)
    exp = ec.primitives("classes", xc, yc)
    assert exp["bad"] == 3 and exp["n"] == 34
    assert_same(got, exp)


def test_update_refusals():
    ev = metrics.Evaluator("multilabel", 5, 16, max_batches=2, device=DEV)
    x, y = torch.zeros(8, 5, device=DEV), torch.zeros(8, 5, device=DEV)
    for bad_x, name in ((x.double(), "logits"), (torch.zeros(8, 4, device=DEV), "logits"), (x.t().contiguous().t(), "logits")):
        with pytest.raises(ValueError, match=name):
            ev.update(bad_x, y)
    for bad_y in (y.long(), torch.zeros(8, device=DEV), torch.zeros(7, 5, device=DEV)):
        with pytest.raises(ValueError, match="target"):
            ev.update(x, bad_y)
    with pytest.raises(ValueError, match="loss"):
        ev.update(x, y, torch.zeros(2, device=DEV))
    with pytest.raises(ValueError, match="gates"):
        ev.update(x, y, None, torch.zeros(7, 3, device=DEV))
    with pytest.raises(RuntimeError, match="no CPU path"):
        ev.update(x.cpu(), y)
    assert ev.n == 0
    with pytest.raises(ValueError, match="no rows"):
        ev.compute()
    ev.update(x, y)
    with pytest.raises(ValueError, match="capacity"):
        ev.update(torch.zeros(9, 5, device=DEV), torch.zeros(9, 5, device=DEV))
    with pytest.raises(ValueError, match="loss"):
        ev.update(x, y, torch.zeros((), device=DEV))              # a loss after a batch without one
    ev.update(x[:4], y[:4])
    with pytest.raises(ValueError, match="max_batches"):
        ev.update(x[:0 + 1], y[:1])
    evc = metrics.Evaluator("classes", 4, 8, device=DEV)
    with pytest.raises(ValueError, match="target"):
        evc.update(torch.zeros(8, 4, device=DEV), torch.zeros(8, device=DEV))           # class indices are int64


def model_args(**kw):
    a = dict(model="mmtrvat", orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=24, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0., res_dropout=0.,
             out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6, bert_model="unused", text_features=True,
             num_vectors_l=32, num_vectors_a=32, num_vectors_v=32, precision="f32", task="mmimdb", task_type="multilabel")
    a.update(kw)
    return SimpleNamespace(**a)


def model_batches(n=3, B=2, Cn=6):
    g = torch.Generator().manual_seed(23)
    zeros = torch.zeros(B, 10, dtype=torch.long)
    return [(torch.randn(B, 10, 32, generator=g), zeros, zeros, torch.randn(B, 20, 35, generator=g),
             (torch.rand(B, Cn, generator=g) > 0.5).float(), torch.randn(B, 30, 74, generator=g)) for _ in range(n)]


def test_model_eval_end_to_end_and_inside_fit(tmp_path):
    from bpmult_amd.models import get_model
    from bpmult_amd.optim import FusedAdam
    torch.manual_seed(29)
    args = model_args()
    model = get_model(args).cuda().eval()
    batches = model_batches()
    crit = losses.BCEWithLogitsLoss()
    seen = []

    def recording(out, tgt):
        loss = crit(out, tgt)
        seen.append((out.detach().clone(), tgt.detach().clone(), loss.detach().clone()))
        return loss

    got = training.model_eval(model, recording, batches, args, output_gates=False)
    x = torch.cat([s[0] for s in seen]).cpu().numpy()
    y = torch.cat([s[1] for s in seen]).cpu().numpy()
    ls = [float(s[2]) for s in seen]
    assert x.shape == (6, 6) and len(ls) == 3
    want = ec.reference_metrics("mmimdb", "multilabel", x, y, ls)
    assert set(got) == set(want)
    for k, w in want.items():
        assert abs(got[k] - w) <= TOL, (k, got[k], w)
    # with the gates kept for the interpretability dump
    ev = metrics.Evaluator("multilabel", 6, 6, device=DEV)
    again = training.model_eval(model, crit, batches, args, evaluator=ev, output_gates=True)
    assert set(again) == set(got) and all(abs(again[k] - got[k]) <= 1e-6 for k in got) and ev.predictions()[3].shape[0] == 6
    # make_evaluate as fit()'s evaluate: two epochs, one Evaluator
    opt = FusedAdam(model, lr=1e-3)
    sched = training.get_scheduler(opt, 2, 0.5)
    ev_fn = training.make_evaluate(crit, lambda: batches, args, "auc_pr_micro")
    r = training.fit(model, opt, sched, lambda: batches, lambda m, b: training.model_forward(m, crit, b, "mmtrvat")[0], ev_fn,
                     str(tmp_path), max_epochs=2, patience=5)
    assert r["epochs_run"] == 2 and r["history"][1]["metric"] == ev_fn.metrics["auc_pr_micro"]
    assert set(ev_fn.metrics) == set(got) and all(np.isfinite(v) for v in ev_fn.metrics.values())
