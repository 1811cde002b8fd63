"""Launch trace of whole model steps, on the CPU: no GPU and no built library.

The toy models run eager steps from HOST tensors (ops._DRY_RUN) against a stand-in for the library that launches nothing
and records every call in order: entry-point name, scalar arguments, every field of every problem struct.  Pointers are
written as (allocation number in order of first use, byte offset) -- resolved WHEN THE CALL IS MADE against the storages
of the tensors alive at that moment (autograd's temporaries are gone when the step ends) -- raw addresses (device
tables, the LayerNorm workspace) likewise, a device-resident dropout seed as a marker.  The record depends on the
launches, not on addresses: two trees that launch the same step print the same bytes.

    python tools/step_trace.py > a.txt          one JSON line per call, one summary line (call counts, SHA-256) per case
    python tools/step_trace.py --summary        the summary lines and the SHA-256 over everything only
    python tools/step_trace.py --shift 12345    the same bytes with every allocation somewhere else

Not in the trace: torch's own ops (zero_, index_select, copy_), graph replay, and the bf16x3 mode (its split images are
allocated on the device); the GPU tests cover those."""
import argparse
import bisect
import ctypes as C
import gc
import hashlib
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bpmult_amd  # noqa: E402,F401
from bpmult_amd import _lib, engine, ops  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402

SIZES = {"bpm_zero_segment_blocks": lambda n: (n + 1023) // 1024 or 1,          # host-side size queries: answered, not recorded
         "bpm_ln_bwd_ws_bytes": lambda n, d: 1 << 16,
         "bpm_adam_blocks": lambda n4: (n4 + 1023) // 1024 or 1}
ONE_STRUCT = (_lib.TailDesc, _lib.TailGrads)                                     # passed by reference, no count behind them


class Recorder:
    """Stands in for the loaded library: every bpm_* entry point records its canonical arguments and returns 0."""

    def __init__(self):
        self.new_case()

    def __getattr__(self, name):
        if not name.startswith("bpm_"):
            raise AttributeError(name)
        if name in SIZES:
            return SIZES[name]
        return lambda *a: self._record(name, a)

    def new_case(self):
        self.calls = []
        self._num = {}              # allocation address -> (bytes, storage id, number in order of first use)
        self._count = 0

    def _live(self):
        live = {}
        for o in gc.get_objects():
            if isinstance(o, torch.Tensor) and o.device.type == "cpu":
                s = o.untyped_storage()
                if s.nbytes():
                    live[s.data_ptr()] = (s.nbytes(), s._cdata)
        for a in [a for a in self._num if a not in live]:                        # freed: its address may be handed out again
            del self._num[a]
        return live, sorted(live)

    def _record(self, name, args):
        live, addrs = self._live()

        def ptr(p):
            if not p:
                return None
            i = bisect.bisect_right(addrs, p) - 1
            if i < 0 or p >= addrs[i] + live[addrs[i]][0]:
                raise ValueError(f"{name}: pointer {p:#x} is in no live allocation")
            a = addrs[i]
            if a not in self._num or self._num[a][:2] != live[a]:
                self._num[a] = live[a] + (self._count,)
                self._count += 1
            return [self._num[a][2], p - a]

        def struct(s):
            out = {}
            for field, ty in s._fields_:
                v = getattr(s, field)
                if ty is C.c_void_p:
                    v = ptr(v)
                elif isinstance(v, C.Array):
                    v = [ptr(x) for x in v] if ty._type_ is C.c_void_p else list(v)
                out[field] = v
            return out

        sig, out = _lib.SIGNATURES[name], []
        assert len(sig) == len(args), (name, len(sig), len(args))
        for i, (a, ty) in enumerate(zip(args, sig)):
            if isinstance(ty, type) and issubclass(ty, C._Pointer):
                if ty._type_ in ONE_STRUCT:
                    out.append(struct(a._obj))
                else:
                    out.append([struct(a[j]) for j in range(args[i + 1])])
            elif ty is C.c_void_p:
                out.append(ptr(a))
            elif ty is C.c_uint64:
                out.append("indirect" if a & _lib.SEED_INDIRECT else int(a))
            else:
                out.append(a)
        self.calls.append([name, out])
        return 0


def _args(model, **kw):                     # tests/test_plan_tables_cpu.py::_args
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=64, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1, res_dropout=0.1,
             out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


FOUR = {"orig_d_a": 96, "num_vectors_a": 40, "num_vectors_v": 40}
ODD = {"hidden_sz": 42, "num_heads": 2}         # B = 1: (B * d) % 4 != 0, the torch path of the two-row additions


def cases():
    """(label, model, constructor overrides, batch size, mode, gates in the loss).  A case is two steps: text length 30,
    then 22 (another key; the tables must not move); in a train case on top of the first step's gradients (the
    accumulating tables).  The first forward of a model refreshes the weight shadows (two launches more)."""
    out = []
    for model, kw in (("mmtrvat", {}), ("mmtrvapt", FOUR)):       # pruned 4-modal: the time maps compute two rows
        for prune in (True, False):
            for prec in ("bf16", "f32"):
                for mode in ("train", "eval"):
                    out.append((f"{model} prune={prune} {prec} {mode}", model, dict(kw, prune_unused_rows=prune, precision=prec),
                                2, mode, True))
    for model, kw in (("mmtrvat", {}), ("mmtrvapt", FOUR)):
        out.append((f"{model} prune=True bf16 train no-gates", model, dict(kw, prune_unused_rows=True), 2, "train", False))
    for prune in (True, False):
        out.append((f"mmtrvat prune={prune} bf16 train hidden 42 B=1", "mmtrvat", dict(ODD, prune_unused_rows=prune), 1, "train", True))
    return out


def run_case(rec, model_name, kw, B, mode, gates):
    """-> [(calls of the step, calls of its forward)] with the records left in rec.calls."""
    torch.manual_seed(1234)                         # dropout seeds are scalar arguments of the launches
    m = get_model(_args(model_name, **kw))
    m.use_graphs = False
    m.train(mode == "train")
    four, a = model_name == "mmtrvapt", _args(model_name, **kw)
    steps = []
    for L in (30, 22):
        x_l = torch.randn(B, L, a.orig_d_l, requires_grad=mode == "train")
        img = torch.randn(B, a.num_vectors_v, a.orig_d_v, requires_grad=mode == "train")
        aud = torch.randn(B, a.num_vectors_a, a.orig_d_a)
        n0 = len(rec.calls)
        with torch.set_grad_enabled(mode == "train"):
            if four:                                # (the audio front-end refuses host tensors: enter behind it)
                logits, z = m._run(x_l, img, aud, torch.randn(B, a.hidden_sz))
            else:
                logits, z = m(x_l, None, None, img, aud, output_gate=True)
        n1 = len(rec.calls)
        if mode == "train":
            (logits.sum() + z.sum() if gates else logits.sum()).backward()
        steps.append((len(rec.calls) - n0, n1 - n0))
        del logits, z, x_l, img, aud
        rec._live()                                 # this step's inputs and outputs are gone: the next one's are new allocations
    return steps


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n")[0])
    ap.add_argument("--summary", action="store_true", help="per-case call counts and digests only")
    ap.add_argument("--shift", type=int, default=0, help="hold an allocation of this many bytes (and a few odd ones) first")
    opt = ap.parse_args()
    rec = Recorder()
    _lib._lib = rec
    ops._DRY_RUN = True
    ops._stream = lambda: 0
    ws = []
    ops._ln_workspace = lambda n, d, device: ws[0]
    torch.cuda.current_device = lambda: 0
    engine._SIDE = False
    gc.collect()
    gc.freeze()                                     # the scans for live tensors only walk what is created from here on
    junk = [torch.empty(opt.shift + 17 * k, dtype=torch.uint8) for k in range(1, 6)] if opt.shift else []
    total = hashlib.sha256()
    ncalls = 0
    for label, model_name, kw, B, mode, gates in cases():
        rec.new_case()
        ws[:] = [torch.zeros(1 << 14)]
        steps = run_case(rec, model_name, kw, B, mode, gates)
        h = hashlib.sha256()
        for i, c in enumerate(rec.calls):
            line = json.dumps([label, i] + c, sort_keys=True, separators=(",", ":"))
            h.update(line.encode() + b"\n")
            if not opt.summary:
                print(line)
        total.update(h.digest())
        ncalls += len(rec.calls)
        print(json.dumps({"case": label, "steps": [{"calls": n, "forward": f} for n, f in steps], "sha256": h.hexdigest()},
                         sort_keys=True))
        gc.collect()
    del junk
    print(json.dumps({"cases": len(cases()), "calls": ncalls, "sha256": total.hexdigest()}, sort_keys=True))


if __name__ == "__main__":
    main()
