#!/usr/bin/env python3
"""Generate the evaluation fixture F17 from the REAL reference: the dict that the reference's own model_eval
(train.py:165-280) returns, scikit-learn and all, for the cases of tests/eval_cases.py.

train.py does not import as shipped here: the modules it imports that are absent (mmbt.*, pytorch_transformers,
pytorch_pretrained_bert, tqdm when missing) are stubbed in sys.modules, and train.model_forward -- which calls .cuda() --
is replaced by a function that hands out the prepared (loss, out, tgt) of each batch.  The losses are torch's CPU
criteria on the batch, as get_criterion builds them unweighted (train.py:99-120).

Per case "<case>.": logits, targets, batch (size), losses (float64, one per batch), and every metric as "m.<key>" float64.
The generator asserts what the cases are built to have: planted logits 0 / 1e-9 / 1e-6 predicting 0 / 0 / 1, two logits
>= 20 tying at 1.0f, reference scores that are a function of the logit and rank as the once-rounded sigmoid does, a class with a single positive, rows without a positive, a ragged last batch, and for the regression
case exact zero targets and predictions more than 1e-3 away from every k + 0.5.

usage:  python tests/golden/make_golden_eval.py
"""
import importlib.machinery
import os
import sys
import types
from argparse import Namespace

import numpy as np

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
sys.path.insert(0, os.path.dirname(HERE))
sys.dont_write_bytecode = True
sys.path.insert(0, "/root/reference")


class _D:
    def __init__(self, *a, **k):
        pass


def _stub(name, **attrs):
    m = types.ModuleType(name)
    m.__spec__ = importlib.machinery.ModuleSpec(name, None)
    m.__path__ = []
    m.__dict__.update(attrs)
    sys.modules[name] = m


for _n, _a in [("mmbt", {}), ("mmbt.data", {}), ("mmbt.data.helpers", {"get_data_loaders": _D}), ("mmbt.models", {"get_model": _D}),
               ("mmbt.models.vilbert", {"BertConfig": _D}), ("mmbt.utils", {}), ("mmbt.utils.logger", {"create_logger": _D}),
               ("mmbt.utils.utils", {"__all__": []}),
               ("pytorch_transformers", {}),
               ("pytorch_transformers.optimization", {"AdamW": _D, "WarmupConstantSchedule": _D, "WarmupLinearSchedule": _D}),
               ("pytorch_pretrained_bert", {"BertAdam": _D}), ("pytorch_pretrained_bert.modeling", {"WEIGHTS_NAME": "pytorch_model.bin"})]:
    _stub(_n, **_a)
try:
    import tqdm  # noqa: F401
except ImportError:
    _stub("tqdm", tqdm=lambda it, **k: it)

_env = {k: os.environ.get(k) for k in ("CUDA_DEVICE_ORDER", "CUDA_VISIBLE_DEVICES")}
import torch  # noqa: E402
import bpmult.train as train  # noqa: E402  (sets the two CUDA_* variables on import)

for _k, _v in _env.items():
    if _v is None:
        os.environ.pop(_k, None)
    else:
        os.environ[_k] = _v

import eval_cases as ec  # noqa: E402


def run_case(case):
    task, task_type, N, C, bs = ec.CASES[case]
    kind = ec.kind_of(task, task_type)
    x, y = ec.make_inputs(case)
    crit = torch.nn.BCEWithLogitsLoss() if kind == "multilabel" else torch.nn.L1Loss() if kind == "regression" else torch.nn.CrossEntropyLoss()
    spans = ec.batches_of(N, bs)
    assert spans[-1][1] - spans[-1][0] not in (0, bs), "the last batch must be ragged"
    prepared = []
    for lo, hi in spans:
        out, tgt = torch.from_numpy(x[lo:hi].copy()), torch.from_numpy(y[lo:hi].copy())
        prepared.append((crit(out, tgt), out, tgt))
    it = iter(prepared)
    train.model_forward = lambda i_epoch, model, args, criterion, batch, gmu_gate=False: next(it)
    args = Namespace(task=task, task_type=task_type)
    metrics = train.model_eval(0, spans, None, args, crit)
    # what the case is built to have
    if kind == "multilabel":
        s = torch.sigmoid(torch.from_numpy(x)).numpy()
        assert (s[0, 0] > 0.5, s[1, 0] > 0.5, s[2, 0] > 0.5) == (False, False, True)
        assert x[3, 0] != x[4, 0] and s[3, 0] == s[4, 0] == np.float32(1.0)
        assert np.array_equal(s > 0.5, ec.sigmoid32(x) > np.float32(0.5))
        # the reference's scores (sigmoid of each batch, as model_eval takes it) are a function of the logit, and rank as
        # the once-rounded sigmoid does: the fixture does not depend on whose sigmoid ran
        sb = np.vstack([torch.sigmoid(p[1]).numpy() for p in prepared])
        for v in np.unique(x):
            assert len(np.unique(sb[x == v])) == 1, f"the reference's sigmoid of {v} depends on the element's position"
        order = np.argsort(x, axis=None, kind="stable")
        assert np.array_equal(np.diff(sb.ravel()[order]) > 0, np.diff(ec.sigmoid32(x).ravel()[order]) > 0)
        assert y[:, C - 1].sum() == 1 and (y.sum(1) == 0).sum() >= 2
        assert 0.15 < y[:, :C - 1].mean() < 0.45            # about 30 % apart from the single-positive class
        if case == "mmimdb_empty":
            assert y[:, 2].sum() == 0
        grid = np.ones_like(x, dtype=bool)
        grid[[0, 1, 2, 3, 4], 0] = False
        assert np.array_equal(x[grid] * 8, np.rint(x[grid] * 8)) and np.abs(x[grid]).max() <= 6
    elif kind == "regression":
        assert ec.regression_ok(x).all() and (y == 0).sum() >= 5
        assert np.array_equal(y * 4, np.rint(y * 4)) and np.abs(y).max() <= 3
    out = {f"{case}.logits": x, f"{case}.targets": y, f"{case}.batch": np.int64(bs),
           f"{case}.losses": np.array([float(p[0].item()) for p in prepared], dtype=np.float64)}
    for k, v in metrics.items():
        out[f"{case}.m.{k}"] = np.float64(v)
    return out


def main():
    import sklearn
    import warnings
    print("scikit-learn", sklearn.__version__)
    out = {}
    with warnings.catch_warnings():
        warnings.simplefilter("ignore")            # "no positive class" of the empty class, on purpose
        for case in ec.CASES:
            out.update(run_case(case))
            print(case, {k.split(".m.")[1]: float(v) for k, v in out.items() if k.startswith(case + ".m.")})
    np.savez_compressed(os.path.join(HERE, "f17_eval.npz"), **out)


if __name__ == "__main__":
    torch.set_num_threads(4)
    main()
