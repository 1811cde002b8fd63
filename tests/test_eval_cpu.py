"""No-GPU checks of the evaluation path: the three bpm_eval_* entries are declared, exported and bound; every invalid
call is refused on the host with nothing launched; the Python layer's refusals; and the numpy restatement of the metrics
(tests/eval_cases.py) and training.arrange_metrics reproduce the fixture that the reference's own model_eval and
scikit-learn produced (tests/golden/f17_eval.npz)."""
import ctypes as C
import math
import os
import re
from types import SimpleNamespace

import numpy as np
import pytest
import torch

import bpmult_amd  # noqa: F401
import eval_cases as ec
from bpmult_amd import _lib, metrics, ops, training

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bpmult_hip.h")).read()
FIX = np.load(os.path.join(ROOT, "tests", "golden", "f17_eval.npz"))
ARG, ALIGN = -1, -2
F32_KEYS = ("mae", "corr", "weight_f1")          # the reference computes these from float32 numpy arrays


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def fixture_metrics(case):
    pfx = case + ".m."
    return {k[len(pfx):]: float(FIX[k]) for k in FIX.files if k.startswith(pfx)}


def test_entries_are_declared_exported_and_bound(lib):
    assert "eval.hip" in _lib.SOURCES
    for name in ("bpm_eval_ws_bytes", "bpm_eval_update", "bpm_eval_finalize"):
        assert re.search(r"^\s*(?:int|size_t)\s+%s\s*\(" % name, HEADER, flags=re.M), name
        assert name in _lib.SIGNATURES and hasattr(lib, name)
    assert lib.bpm_version() == 5 and "#define BPM_ABI_VERSION 5" in HEADER
    body = re.search(r"typedef struct bpm_eval_desc \{(.*?)\} bpm_eval_desc;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in filter(None, (d.strip() for d in body.split(";"))):
        parts = decl.split(",")
        names += [parts[0].split()[-1].lstrip("*")] + [p.strip().lstrip("*") for p in parts[1:]]
    assert names == [f[0] for f in _lib.EvalDesc._fields_]
    kinds = re.search(r"enum \{ BPM_EVAL_MULTILABEL = (\d), BPM_EVAL_REGRESSION = (\d), BPM_EVAL_CLASSES = (\d) \}", HEADER).groups()
    assert tuple(int(k) for k in kinds) == (_lib.EVAL_MULTILABEL, _lib.EVAL_REGRESSION, _lib.EVAL_CLASSES)


def test_ws_bytes(lib):
    ws = lib.bpm_eval_ws_bytes
    cdiv = lambda a, b: (a + b - 1) // b                  # noqa: E731
    for N, Cn in ((1, 1), (37, 5), (300, 23), (8192, 23)):
        nq = cdiv(N * Cn, 1024) + Cn * cdiv(N, 1024)
        assert ws(_lib.EVAL_MULTILABEL, N, Cn) == 16 * N * Cn + 16 * nq + 24 * cdiv(N, 256)
        assert ws(_lib.EVAL_REGRESSION, N, 1) == ws(_lib.EVAL_CLASSES, N, Cn) == cdiv(N, 1024) * 14 * 8
    assert ws(_lib.EVAL_MULTILABEL, 8192, 23) % 8 == 0
    assert ws(3, 8, 2) == 0 and ws(-1, 8, 2) == 0 and ws(0, 0, 2) == 0 and ws(0, 8, 0) == 0
    assert ws(_lib.EVAL_MULTILABEL, 1 << 20, 1 << 11) == 0           # 2^31 elements
    assert ws(_lib.EVAL_MULTILABEL, 1 << 20, 2047) > 0


def valid_desc(kind, Cn=4, cap=64):
    """A descriptor that passes validation, over made-up aligned addresses: only REFUSED calls are made with it."""
    d = _lib.EvalDesc()
    d.kind, d.C, d.capacity, d.max_batches = kind, 1 if kind == _lib.EVAL_REGRESSION else Cn, cap, 8
    d.score, d.predict, d.raw, d.target = 0x10000, 0x20000, 0x30000, 0x40000
    d.pred, d.label, d.losses, d.bad = 0x50001, 0x60003, 0x70000, 0x80000
    d.logits, d.ld, d.targets, d.ldt, d.loss = 0x90000, d.C, 0xA0000, d.C, 0xB0000
    d.B, d.n0, d.batch_index = 8, 56, 7
    d.N, d.nbatches, d.result, d.counts, d.ws, d.ws_bytes = cap, 8, 0xC0000, 0xD0000, 0xE0000, 1 << 24
    return d


def refused(lib, fn, d, field, value, code):
    old = getattr(d, field)
    setattr(d, field, value)
    rc = getattr(lib, fn)(C.byref(d), None)
    setattr(d, field, old)
    assert rc == code, (fn, d.kind, field, value, rc)


@pytest.mark.parametrize("kind", [0, 1, 2])
def test_invalid_calls_are_refused_before_any_launch(lib, kind):
    assert lib.bpm_eval_update(None, None) == ARG and lib.bpm_eval_finalize(None, None) == ARG
    d = valid_desc(kind)
    used = {0: ("score", "pred", "label"), 1: ("score", "predict", "raw", "target"), 2: ("predict", "target", "label")}[kind]
    for fn in ("bpm_eval_update", "bpm_eval_finalize"):
        refused(lib, fn, d, "kind", 3, ARG)
        refused(lib, fn, d, "kind", -1, ARG)
        for f in used:
            refused(lib, fn, d, f, None, ARG)
        refused(lib, fn, d, "C", 0, ARG)
        refused(lib, fn, d, "capacity", 0, ARG)
        for f in ("score", "predict", "raw", "target", "losses", "bad"):
            refused(lib, fn, d, f, getattr(d, f) + 2, ALIGN)
    up = "bpm_eval_update"
    refused(lib, up, d, "logits", None, ARG)
    refused(lib, up, d, "targets", None, ARG)
    refused(lib, up, d, "B", 0, ARG)
    refused(lib, up, d, "B", 9, ARG)                        # n0 + B > capacity
    refused(lib, up, d, "n0", 57, ARG)
    refused(lib, up, d, "n0", -1, ARG)
    refused(lib, up, d, "ld", d.C - 1, ARG)
    refused(lib, up, d, "batch_index", 8, ARG)              # >= max_batches
    refused(lib, up, d, "batch_index", -1, ARG)
    refused(lib, up, d, "losses", None, ARG)                # a loss needs the loss array
    refused(lib, up, d, "logits", d.logits + 2, ALIGN)
    refused(lib, up, d, "loss", d.loss + 1, ALIGN)
    refused(lib, up, d, "targets", d.targets + (4 if kind == 2 else 2), ALIGN)     # int64 class indices: 8-byte aligned
    if kind == 0:
        refused(lib, up, d, "ldt", d.C - 1, ARG)
    if kind == 1:
        refused(lib, up, d, "C", 2, ARG)
    fin = "bpm_eval_finalize"
    refused(lib, fin, d, "N", 0, ARG)
    refused(lib, fin, d, "N", d.capacity + 1, ARG)
    refused(lib, fin, d, "nbatches", 9, ARG)
    refused(lib, fin, d, "nbatches", -1, ARG)
    refused(lib, fin, d, "result", None, ARG)
    refused(lib, fin, d, "counts", None, ARG)
    refused(lib, fin, d, "ws", None, ARG)
    refused(lib, fin, d, "ws_bytes", lib.bpm_eval_ws_bytes(kind, d.N, d.C) - 1, ARG)
    refused(lib, fin, d, "ws", d.ws + 4, ALIGN)
    refused(lib, fin, d, "result", d.result + 4, ALIGN)
    refused(lib, fin, d, "counts", d.counts + 4, ALIGN)


def test_python_refusals():
    with pytest.raises(ValueError, match="kind"):
        metrics.Evaluator("ranking", 3, 8)
    with pytest.raises(ValueError, match="num_classes"):
        metrics.Evaluator("regression", 3, 8)
    with pytest.raises(ValueError, match="capacity"):
        metrics.Evaluator("multilabel", 3, 0)
    with pytest.raises(ValueError, match="max_batches"):
        metrics.Evaluator("multilabel", 3, 8, max_batches=0)
    with pytest.raises(RuntimeError, match="no CPU path"):
        metrics.Evaluator("multilabel", 3, 8, device="cpu")
    with pytest.raises(ValueError, match="eval.score: expected float32"):
        ops.eval_desc(0, 3, 8, score=torch.zeros(8, 3, dtype=torch.float64))
    with pytest.raises(ValueError, match="eval.pred: expected uint8"):
        ops.eval_desc(0, 3, 8, pred=torch.zeros(8, 3, dtype=torch.int32))
    with pytest.raises(ValueError, match="no CPU fallback"):
        ops.eval_desc(0, 3, 8, score=torch.zeros(8, 3))
    with pytest.raises(ValueError, match="cmu-mosi"):
        training.eval_kind(SimpleNamespace(task="cmu-mosi", task_type="multilabel"))
    with pytest.raises(ValueError, match="cmu-mosi"):
        training.model_eval(None, None, [], SimpleNamespace(task="cmu-mosi", task_type="multilabel", model="mmtrvat", n_classes=1))
    x, y = ec.make_inputs("mmimdb")
    prim = ec.primitives("multilabel", x, y, [1.0])
    with pytest.raises(ValueError, match="exactly 6"):
        training.arrange_metrics(SimpleNamespace(task="cmu-mosei", task_type="multilabel"), prim)
    with pytest.raises(ValueError, match="exactly 2"):
        training.arrange_metrics(SimpleNamespace(task="counseling", task_type="multilabel"), prim)
    assert training.eval_kind(SimpleNamespace(task="cmu-mosi", task_type="classification")) == "regression"
    assert training.eval_kind(SimpleNamespace(task="iemocap", task_type="classification")) == "classes"
    assert training.eval_kind(SimpleNamespace(task="mmimdb", task_type="multilabel")) == "multilabel"


def test_weighted_accuracy_is_nan_where_the_reference_divides_by_zero():
    wacc, wf1 = metrics.weighted_accuracy([3, 0, 2], [1, 2, 0], [2, 0, 1], [4, 8, 0])      # class 1: no positive; class 2: no negative
    assert math.isnan(wacc[1]) and math.isnan(wf1[1]) and math.isnan(wacc[2]) and math.isnan(wf1[2])
    assert wacc[0] == (3 * 5 / 5 + 4) / 10
    e_wacc, e_wf1 = ec.weighted_acc([3, 0, 2], [1, 2, 0], [2, 0, 1], [4, 8, 0])
    assert np.array_equal(wacc, e_wacc, equal_nan=True) and np.array_equal(wf1, e_wf1, equal_nan=True)


@pytest.mark.parametrize("case", list(ec.CASES))
def test_fixture_inputs_are_the_named_ones(case):
    x, y = ec.make_inputs(case)
    assert np.array_equal(x, FIX[case + ".logits"]) and np.array_equal(y, FIX[case + ".targets"])
    task, task_type, N, Cn, bs = ec.CASES[case]
    assert int(FIX[case + ".batch"]) == bs and len(FIX[case + ".losses"]) == len(ec.batches_of(N, bs)) and N % bs


@pytest.mark.parametrize("case", list(ec.CASES))
def test_restatement_reproduces_every_fixture_metric(case):
    """1e-12 for the fp64 metrics; 1e-5 relative for mae / corr, which the reference computes from float32 numpy arrays
    (pairwise float32 summation over 300 terms plus the two fp32 roundings of predict: about 1e-6)."""
    task, task_type, N, Cn, bs = ec.CASES[case]
    want = fixture_metrics(case)
    got = ec.reference_metrics(task, task_type, FIX[case + ".logits"], FIX[case + ".targets"], FIX[case + ".losses"])
    assert set(got) == set(want)
    for k, w in want.items():
        if k in F32_KEYS and task_type != "multilabel":
            assert abs(got[k] - w) <= 1e-5 * abs(w), (k, got[k], w)
        else:
            assert abs(got[k] - w) <= 1e-12, (k, got[k], w)


@pytest.mark.parametrize("case", list(ec.CASES))
def test_model_eval_keys_per_task_are_the_reference_s(case):
    """training.arrange_metrics over the restated primitives: the fixture's keys (plus `acc` for the cross-entropy tasks)
    and the fixture's values."""
    task, task_type, N, Cn, bs = ec.CASES[case]
    kind = ec.kind_of(task, task_type)
    prim = ec.primitives(kind, FIX[case + ".logits"], FIX[case + ".targets"], FIX[case + ".losses"])
    got = training.arrange_metrics(SimpleNamespace(task=task, task_type=task_type), prim)
    want = fixture_metrics(case)
    assert set(got) == set(want) | ({"acc"} if kind == "classes" else set())
    assert list(got)[:len(want)] == [k[len(case) + 3:] for k in FIX.files if k.startswith(case + ".m.")] or kind == "classes"
    for k, w in want.items():
        tol = 1e-5 * abs(w) if k in F32_KEYS and task_type != "multilabel" else 1e-12
        assert abs(got[k] - w) <= tol, (k, got[k], w)
