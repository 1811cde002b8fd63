"""Canonical digest of every EncoderGroupPlan launch table, built from host tensors (ops._DRY_RUN, as the CPU tests do).

One JSON line per plan: every step of the forward, backward and unfold tables (stream placement and function names
included), every field of every problem struct, pointers as (allocation number, byte offset), the x3 flags and presplit
sets, and the bytes the plan owns.  Allocations are the distinct storages reachable from the plan's and the store's
attributes, numbered in order of first use, so the digest ignores buffer names and allocation order but not aliasing.
Two trees that build the same tables print the same bytes:  python tools/plan_digest.py > a.txt  (needs a built library)."""
import ctypes as C
import itertools
import json
import os
import sys
from types import SimpleNamespace

import torch

sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
import bpmult_amd  # noqa: E402,F401
from bpmult_amd import engine, ops  # noqa: E402
from bpmult_amd._lib import BPM_BF16, UnfoldDesc  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.models.encoder import TransformerEncoder  # noqa: E402


def _storages(obj, out, seen):
    if isinstance(obj, torch.Tensor):
        s = obj.untyped_storage()
        out[s.data_ptr()] = s.nbytes()
    elif isinstance(obj, dict) and id(obj) not in seen:
        seen.add(id(obj))
        for v in obj.values():
            _storages(v, out, seen)
    elif isinstance(obj, (list, tuple)) and id(obj) not in seen:
        seen.add(id(obj))
        for v in obj:
            _storages(v, out, seen)
    return out


def digest(plan):
    owned = _storages(vars(plan), {}, set())
    allocs = sorted({**_storages(vars(plan.store), {}, set()), **owned}.items())
    num = {}

    def ptr(p):
        if not p:
            return None
        for a, n in allocs:
            if a <= p < a + n:
                return [num.setdefault(a, len(num)), p - a]
        raise ValueError(f"pointer {p:#x} is in no allocation of the plan or its store")

    def struct(s):
        out = {}
        for name, ty in s._fields_:
            v = getattr(s, name)
            if ty is C.c_void_p:
                v = ptr(v)
            elif isinstance(v, C.Array):
                v = [ptr(x) for x in v] if ty._type_ is C.c_void_p else list(v)
            out[name] = v
        return out

    def arg(a):
        if isinstance(a, C.Array):
            d = {"probs": [struct(s) for s in a]}
            if hasattr(a, "x3"):
                d["x3"] = bool(a.x3)
                d["presplit"] = sorted(ptr(p) for p in a.x3_presplit)
            return d
        if isinstance(a, (int, float, str, bool)) or a is None:
            return a
        if isinstance(a, torch.Tensor):                  # a table a launch reads (kv_source_fwd / _bwd: the position table)
            return {"tensor": ptr(a.data_ptr()), "shape": list(a.shape), "dtype": str(a.dtype)}
        raise TypeError(f"unexpected step argument {type(a)}")

    def step(s):
        if s is engine.JOIN:
            return "join"
        if s[0] in (engine.SIDE, engine.SIDE2):
            return [s[0], step(s[1])]
        if s[0] in (engine.MARK, engine.WAIT):
            return list(s)
        if s[0] is ops.unfold_grads:             # (fn, device table, n, blocks, stores)
            tab, n = s[1], s[2]
            descs = [struct(UnfoldDesc.from_buffer_copy(bytes(tab.cpu().numpy()), k * C.sizeof(UnfoldDesc))) for k in range(n)]
            return [s[0].__name__, descs] + [arg(a) for a in s[2:]]
        return [s[0].__name__] + [arg(a) for a in s[1:]]

    d = {"fwd": {str(t): [step(s) for s in plan._fwd[t]] for t in (True, False)},
         "bwd": {f"{t},{f}": [step(s) for s in plan._bwd[(t, f)]] for t in (True, False) for f in (True, False)},
         "unfold": [[step((ops.unfold_grads,) + u)] for u in plan._unfold],
         "owned_bytes": sum(n for a, n in owned.items() if a not in _storages(vars(plan.store), {}, set()))}
    return d


def _args(model, base, **kw):
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=base[0], vonly=True, lonly=True,
             aonly=True, num_heads=base[1], layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1,
             res_dropout=0.1, out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


def _emit(label, plan):
    print(json.dumps({"plan": label, **digest(plan)}, sort_keys=True, separators=(",", ":")))


def main():
    ops._DRY_RUN = True
    precs = ("bf16", "f32", "bf16x3")
    four = {"orig_d_a": 96, "num_vectors_a": 40, "num_vectors_v": 40}
    models = [(base, m, kw) for base, wide in (((64, 4), (40, None)), ((512, 2), (384, 272)))
              for m, kw in (("mmtrvat", {}), ("mmtrvat", {"hidden_sz": wide[0]}), ("mmtrvapt", four),
                            ("mmtrvapt", {**four, "hidden_sz": wide[1] or wide[0]}))]
    for (base, m, kw), prune, prec, lowrank, dkv in itertools.product(models, (True, False), precs, (True, False),
                                                                       ("auto", "0", "1", "2")):
        engine._LOWRANK, engine._DKV_SIDE_ENV = lowrank, dkv
        model = get_model(_args(m, base, prune_unused_rows=prune, **{**kw, "precision": prec}))
        model._ensure_store()
        trunk = model._trunk_for(2)
        for k, plan in (("plan1", trunk.plan1), ("plan2", trunk.plan2)):
            _emit(f"{m} {base} {kw} prune={prune} {prec} lowrank={lowrank} dkv={dkv} {k}", plan)
    engine._LOWRANK, engine._DKV_SIDE_ENV = True, "auto"
    for (d, H, L, Tn), bi, prec in itertools.product([(24, 4, 2, 9), (24, 4, 2, 7), (50, 2, 3, 70), (512, 2, 1, 40)],
                                                     (False, True), precs):
        enc = TransformerEncoder(d, H, L, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.1,
                                 attn_mask=True, biprojection=bi)
        enc.precision = prec
        x = torch.zeros(Tn, 2, d)
        for form, xk in (("self", None), ("cross", x)):
            _emit(f"encoder d={d} H={H} L={L} T={Tn} bi={bi} {prec} {form}", enc._plan_for(x, xk))
    for bi, (dt, x3) in itertools.product((False, True), ((BPM_BF16, False), (0, False), (0, True))):
        d, H, L, B = 24, 4, 2, 2
        encs = [TransformerEncoder(d, H, L, attn_mask=True, biprojection=bi) for _ in range(3)]
        st = engine.ParamStore([(f"e{j}.{k}", p) for j, m in enumerate(encs) for k, p in m.named_parameters()], dt, x3=x3)
        for j in range(3):
            engine.register_encoder_shadows(st, f"e{j}.", d, L, biprojection=bi)
        st.finalize_shadows()
        cfg = engine.GroupCfg(d, H, L, 0.1, 0.1, 0.1, True, bi, self_only=True)
        plan = engine.EncoderGroupPlan(st, cfg, [engine.EncoderDesc(f"e{j}.", j, n, n, 0.1) for j, n in enumerate((5, 9, 6))], B)
        _emit(f"group of three self-only bi={bi} dtype={dt} x3={x3}", plan)


if __name__ == "__main__":
    main()
