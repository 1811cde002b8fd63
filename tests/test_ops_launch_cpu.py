"""The Python layer between the C ABI and the launch tables, without a GPU and without a built library: a stand-in for the
library records every call.  Chunking of every grouped wrapper at the library's group limits (ops._grouped), the key masks
that travel beside the problems, the dropout seed's way into every seeded entry, the calling convention of the plan steps
(engine.EncoderGroupPlan._exec, ops.SEEDED / ops.STEP_FUNCTIONS) and the three shared argument checks."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, engine, ops
from bpmult_amd._lib import BPM_BF16, GEMM_MAX_GROUP, GEMM_NT, MAX_GROUP
from bpmult_amd.models import get_model
from bpmult_amd.models.encoder import TransformerEncoder

D, SCALE, SEED = 8, 2.0, 0x1234_5678_9ABC
TABLE = torch.zeros(4, D)


class Recorder:
    """Stands in for the loaded library: size queries are answered, every other bpm_* entry records (name, args) -> 0."""
    SIZES = {"bpm_zero_segment_blocks": lambda n: (n + 4095) // 4096, "bpm_ln_bwd_ws_bytes": lambda n, d: 1 << 10}

    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("bpm_"):
            raise AttributeError(name)
        return self.SIZES.get(name) or (lambda *a: self.calls.append((name, a)) or 0)


@pytest.fixture
def rec(monkeypatch):
    r, ws = Recorder(), torch.zeros(1 << 8)
    monkeypatch.setattr(_lib, "_lib", r)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_DRY_RUN", True)
    monkeypatch.setattr(ops, "_DRY_LAUNCHES", [])
    monkeypatch.setattr(ops, "_ln_workspace", lambda n, d, device: ws)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    return r


def _masks(p):
    return (_lib.AttnKMask * len(p))()


# ops function -> (entry point, the call with a problem array and the keywords under test)
GROUPED = {
    ops.gemm_grouped: ("bpm_gemm_grouped", lambda p, **k: ops.gemm_grouped(BPM_BF16, GEMM_NT, p, **k)),
    ops._split: ("bpm_split_rows", lambda p: ops._split(p)),
    ops.attn_fwd: ("bpm_attn_fwd", lambda p, **k: ops.attn_fwd(BPM_BF16, p, **k)),
    ops.attn_bwd: ("bpm_attn_bwd", lambda p, **k: ops.attn_bwd(BPM_BF16, p, **k)),
    ops.attn_bwd_dq: ("bpm_attn_bwd_dq", lambda p, **k: ops.attn_bwd_dq(BPM_BF16, p, **k)),
    ops.attn_bwd_dkv: ("bpm_attn_bwd_dkv", lambda p, **k: ops.attn_bwd_dkv(BPM_BF16, p, **k)),
    ops.attn_fwd_kmask: ("bpm_attn_fwd_kmask", lambda p, **k: ops.attn_fwd_kmask(BPM_BF16, p, _masks(p), **k)),
    ops.attn_bwd_dq_kmask: ("bpm_attn_bwd_dq_kmask", lambda p, **k: ops.attn_bwd_dq_kmask(BPM_BF16, p, _masks(p), **k)),
    ops.attn_bwd_dkv_kmask: ("bpm_attn_bwd_dkv_kmask", lambda p, **k: ops.attn_bwd_dkv_kmask(BPM_BF16, p, _masks(p), **k)),
    ops.attn_maps: ("bpm_attn_maps", lambda p: ops.attn_maps(BPM_BF16, p)),
    ops.pack_rows_fwd: ("bpm_pack_rows_fwd", lambda p, **k: ops.pack_rows_fwd(BPM_BF16, p, **k)),
    ops.pack_rows_bwd: ("bpm_pack_rows_bwd", lambda p, **k: ops.pack_rows_bwd(p, **k)),
    ops.embed_pos_fwd: ("bpm_embed_pos_fwd", lambda p, **k: ops.embed_pos_fwd(p, TABLE, D, SCALE, **k)),
    ops.embed_pos_bwd: ("bpm_embed_pos_bwd", lambda p, **k: ops.embed_pos_bwd(p, D, SCALE, **k)),
    ops.kv_source_fwd: ("bpm_kv_source_fwd", lambda p, **k: ops.kv_source_fwd(BPM_BF16, p, TABLE, D, SCALE, **k)),
    ops.kv_source_bwd: ("bpm_kv_source_bwd", lambda p, **k: ops.kv_source_bwd(p, TABLE, D, SCALE, **k)),
    ops.ln_fwd: ("bpm_ln_fwd", lambda p: ops.ln_fwd(BPM_BF16, p, D)),
    ops.ln_bwd: ("bpm_ln_bwd_ws", lambda p, **k: ops.ln_bwd(p, D, BPM_BF16, **k)),
    ops.rows_cast: ("bpm_rows_cast", lambda p, **k: ops.rows_cast(BPM_BF16, p, **k)),
    ops.gelu_fwd: ("bpm_gelu_fwd", lambda p: ops.gelu_fwd(BPM_BF16, p)),
    ops.gelu_bwd: ("bpm_gelu_bwd", lambda p: ops.gelu_bwd(BPM_BF16, p)),
    ops.expand_heads: ("bpm_expand_heads", lambda p: ops.expand_heads(BPM_BF16, p)),
    ops.add_n: ("bpm_add_n", lambda p: ops.add_n(p)),
    ops.gmu2_fwd: ("bpm_gmu2_fwd", lambda p: ops.gmu2_fwd(p, D)),
    ops.gmu2_bwd: ("bpm_gmu2_bwd", lambda p: ops.gmu2_bwd(BPM_BF16, p, D)),
}
# seeded launches of one struct passed by reference
SINGLE = {
    ops.bert_embed_fwd: ("bpm_bert_embed_fwd", lambda p, **k: ops.bert_embed_fwd(BPM_BF16, _lib.BertEmbedProblem(), D, 1e-5, **k)),
    ops.tail_fwd: ("bpm_tail_fwd", lambda p, **k: ops.tail_fwd(_lib.TailDesc(), **k)),
}
KMASK = ("bpm_attn_fwd_kmask", "bpm_attn_bwd_dq_kmask", "bpm_attn_bwd_dkv_kmask")


def _struct(name):
    return next(t._type_ for t in _lib.SIGNATURES[name] if isinstance(t, type) and issubclass(t, C._Pointer))


def _addr(pointer):
    return C.cast(pointer, C.c_void_p).value


def _split_args(name, args):
    """-> (problem pointer, mask pointer or None, count, the scalars) of one recorded call."""
    sig = _lib.SIGNATURES[name]
    assert len(args) == len(sig), (name, len(args), len(sig))
    i = next(j for j, t in enumerate(sig) if isinstance(t, type) and issubclass(t, C._Pointer))
    nptr = 2 if name in KMASK else 1
    return args[i], (args[i + 1] if nptr == 2 else None), args[i + nptr], args[:i] + args[i + nptr + 1:]


@pytest.mark.parametrize("fn", list(GROUPED), ids=lambda f: f.__name__)
@pytest.mark.parametrize("twice", [False, True], ids=["limit+1", "2*limit"])
def test_groups_are_split_at_the_limit(rec, monkeypatch, fn, twice):
    name, call = GROUPED[fn]
    if fn is ops.attn_maps:
        monkeypatch.setattr(ops, "_DRY_RUN", False)           # (a dry run records attn_maps instead of launching it)
    limit = GEMM_MAX_GROUP if fn is ops.gemm_grouped else MAX_GROUP
    cls = _struct(name)
    probs = (cls * (2 * limit if twice else limit + 1))()
    call(probs)
    assert [c[0] for c in rec.calls] == [name, name]
    (p0, m0, k0, s0), (p1, m1, k1, s1) = (_split_args(name, c[1]) for c in rec.calls)
    assert (k0, k1) == (limit, limit if twice else 1)
    assert _addr(p0) == C.addressof(probs) and _addr(p1) - _addr(p0) == limit * C.sizeof(cls)
    assert s0 == s1 and len(s0) == len(_lib.SIGNATURES[name]) - (3 if name in KMASK else 2)      # the scalars and the stream
    if name in KMASK:
        assert _addr(m1) - _addr(m0) == limit * C.sizeof(_lib.AttnKMask)


@pytest.mark.parametrize("fn", [ops.attn_fwd_kmask, ops.attn_bwd_dq_kmask, ops.attn_bwd_dkv_kmask], ids=lambda f: f.__name__)
def test_one_key_mask_per_problem(rec, fn):
    probs = (_lib.AttnProblem * (MAX_GROUP + 1))()
    masks = (_lib.AttnKMask * (MAX_GROUP + 1))()
    fn(BPM_BF16, probs, masks, 3)
    (p0, m0, _, _), (p1, m1, _, _) = (_split_args(c[0], c[1]) for c in rec.calls)
    assert _addr(m0) == C.addressof(masks) and _addr(m1) - _addr(m0) == MAX_GROUP * C.sizeof(_lib.AttnKMask)
    assert _addr(p1) - _addr(p0) == MAX_GROUP * C.sizeof(_lib.AttnProblem)
    for n in (MAX_GROUP, MAX_GROUP + 2):
        with pytest.raises(ValueError, match="one key mask per problem"):
            fn(BPM_BF16, probs, (_lib.AttnKMask * n)(), 3)
    assert len(rec.calls) == 2


def test_the_seeded_set_is_covered():
    assert set(ops.SEEDED) == {f for f, (_, call) in {**GROUPED, **SINGLE}.items() if call.__code__.co_flags & 0x08}     # takes **k
    assert ops.SEEDED <= ops.STEP_FUNCTIONS and all(f in ops.STEP_FUNCTIONS for f in GROUPED if f is not ops._split)
    assert {ops.gemm_grouped, ops.attn_fwd, ops.attn_bwd, ops.attn_bwd_dq, ops.attn_bwd_dkv, ops.rows_cast, ops.ln_bwd,
            ops.kv_source_fwd, ops.kv_source_bwd} <= ops.SEEDED


@pytest.mark.parametrize("fn", sorted(ops.SEEDED, key=lambda f: f.__name__), ids=lambda f: f.__name__)
def test_seed_reaches_the_entry(rec, fn):
    name, call = {**GROUPED, **SINGLE}[fn]
    probs = (_struct(name) * 1)()
    with pytest.raises(ValueError, match="63-bit"):
        call(probs, seed=(1 << 63) | 5)                      # a plain int with bit 63 set: refused, not dereferenced
    assert not rec.calls
    call(probs, seed=SEED)
    (got, args), = rec.calls
    sig = _lib.SIGNATURES[name]
    assert got == name and len(args) == len(sig)
    assert args[sig.index(C.c_uint64)] == SEED               # (the seed is the first 64-bit word of every seeded signature)
    dev = ops.DeviceSeed(torch.zeros(1, dtype=torch.int64))   # a device-resident seed keeps its marker bit
    call(probs, seed=dev)
    assert rec.calls[1][1][sig.index(C.c_uint64)] == int(dev) and int(dev) & _lib.SEED_INDIRECT


# ---- plan steps ------------------------------------------------------------------------------------------------------
def _args(model, **kw):                     # tests/test_plan_tables_cpu.py::_args
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=64, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1, res_dropout=0.1,
             out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


def _self_only_group():
    d, H, L, B = 24, 4, 2, 2
    encs = [TransformerEncoder(d, H, L, attn_mask=True) for _ in range(3)]
    st = engine.ParamStore([(f"e{j}.{k}", p) for j, m in enumerate(encs) for k, p in m.named_parameters()], BPM_BF16)
    for j in range(3):
        engine.register_encoder_shadows(st, f"e{j}.", d, L, biprojection=False)
    st.finalize_shadows()
    cfg = engine.GroupCfg(d, H, L, 0.1, 0.1, 0.1, True, False, self_only=True)
    return engine.EncoderGroupPlan(st, cfg, [engine.EncoderDesc(f"e{j}.", j, n, n, 0.1) for j, n in enumerate((5, 9, 6))], B)


def _plans(case):
    if case == "self-only":
        return [_self_only_group()]
    model, prune = case
    kw = {"orig_d_a": 96, "num_vectors_a": 40, "num_vectors_v": 40} if model == "mmtrvapt" else {}
    m = get_model(_args(model, prune_unused_rows=prune, **kw))
    m._ensure_store()
    trunk = m._trunk_for(2)
    return [trunk.plan1, trunk.plan2]


@pytest.mark.parametrize("case", [("mmtrvat", True), ("mmtrvat", False), ("mmtrvapt", True), ("mmtrvapt", False), "self-only"],
                         ids=lambda c: c if isinstance(c, str) else f"{c[0]}-{'pruned' if c[1] else 'dense'}")
def test_every_plan_step_runs_through_one_convention(rec, case):
    entry = lambda fn: "bpm_ln_bwd_ws" if fn is ops.ln_bwd else "bpm_" + fn.__name__
    seen, fns = set(), set()
    for plan in _plans(case):
        rec.calls.clear()                                    # (building the store refreshes the weight shadows)
        for steps in (*plan._fwd.values(), *plan._bwd.values()):
            for s in steps:
                if s is engine.JOIN or s[0] in (engine.MARK, engine.WAIT):
                    continue
                s = s[1] if s[0] in (engine.SIDE, engine.SIDE2) else s
                assert s[0] in ops.STEP_FUNCTIONS, s[0]
                if id(s) in seen:
                    continue
                seen.add(id(s))
                fns.add(s[0])
                n0 = len(rec.calls)
                plan._exec(s, SEED)
                new = rec.calls[n0:]
                assert new and {c[0] for c in new} == {entry(s[0])}, (s[0].__name__, [c[0] for c in new])
                sig = _lib.SIGNATURES[entry(s[0])]
                assert all(len(c[1]) == len(sig) for c in new)
                if s[0] in ops.SEEDED:
                    assert all(c[1][sig.index(C.c_uint64)] == SEED for c in new)
                if s[0] is ops.ln_bwd:                      # the step carries its dtype: nothing is completed by the executor
                    assert s[3] == plan.dtype and all(c[1][0] == plan.dtype for c in new)
    assert {ops.gemm_grouped, ops.ln_fwd, ops.ln_bwd} <= fns


def test_a_foreign_step_is_refused_when_the_tables_are_built(rec, monkeypatch):
    build = engine.EncoderGroupPlan._build_fwd
    monkeypatch.setattr(engine.EncoderGroupPlan, "_build_fwd", lambda self, training: build(self, training) + [(print, 1)])
    with pytest.raises(ValueError, match="print"):
        _self_only_group()
    monkeypatch.setattr(engine.EncoderGroupPlan, "_build_fwd", lambda self, training: [(engine.SIDE, (len, 1))] + build(self, training))
    with pytest.raises(ValueError, match="len"):
        _self_only_group()


# ---- the shared argument checks ----------------------------------------------------------------------------------------
def _bert_embed(**kw):
    B, L, f = 2, 3, lambda *s: torch.zeros(*s)
    a = dict(ids=torch.zeros(B, L, dtype=torch.int64), seg=None, word=f(5, D), pos=f(4, D), typ=f(2, D), gamma=f(D), beta=f(D),
             x=f(L * B, D), s=f(L * B, D), mean=f(L * B), rstd=f(L * B), bad=torch.zeros(1, dtype=torch.int32))
    a.update(kw)
    pos = [a.pop(k) for k in ("ids", "seg", "word", "pos", "typ", "gamma", "beta")]
    return ops.bert_embed_problem(*pos, **a)


def test_int32_device_counters(rec):
    assert _bert_embed().bad
    for bad in (torch.zeros(1), torch.zeros(1, dtype=torch.int64), torch.zeros(0, dtype=torch.int32)):
        with pytest.raises(ValueError, match="bert_embed.bad: an int32 device counter"):
            _bert_embed(bad=bad)
        with pytest.raises(ValueError, match="loss.bad: an int32 device counter"):
            ops.loss_problem(_lib.LOSS_CE, _lib.LOSS_MEAN, None, None, None, 2, 3, bad=bad)
        with pytest.raises(ValueError, match="eval.bad: an int32 device counter"):
            ops.eval_desc(_lib.EVAL_CLASSES, 3, 8, bad=bad)
    ok = torch.zeros(1, dtype=torch.int32)
    assert ops.loss_problem(_lib.LOSS_CE, _lib.LOSS_MEAN, None, None, None, 2, 3, bad=ok).bad == ok.data_ptr()
    assert ops.eval_desc(_lib.EVAL_CLASSES, 3, 8, bad=ok).bad == ok.data_ptr()


def test_float32_row_tables(rec):
    one = lambda cls: (cls * 1)()
    wrong = [TABLE.double(), torch.zeros(4, D + 1), torch.zeros(4, 2 * D)[:, :D], torch.zeros(4 * D)]
    for t in wrong:
        for call in (lambda: ops.embed_pos_fwd(one(_lib.EmbedProblem), t, D, SCALE), lambda: ops.kv_source_fwd(BPM_BF16, one(_lib.KvSourceProblem), t, D, SCALE),
                     lambda: ops.kv_source_bwd(one(_lib.KvSourceProblem), t, D, SCALE)):
            with pytest.raises(ValueError, match="expected float32"):
                call()
    for key in ("word", "pos", "typ"):
        for t in (TABLE.double(), torch.zeros(4, 2 * D)[:, :D]):
            with pytest.raises(ValueError, match="bert_embed.*expected float32"):
                _bert_embed(**{key: t})
    assert not rec.calls
    rows = torch.zeros(6, D)[1:5]                           # a view of whole rows is a table
    ops.embed_pos_fwd(one(_lib.EmbedProblem), rows, D, SCALE)
    assert rec.calls[0][1][2:5] == (rows.data_ptr(), 4, D) and _bert_embed(word=rows).word == rows.data_ptr()


def test_adam_device_scalars(rec):
    f, i32 = torch.zeros(4), lambda n: torch.zeros(n, dtype=torch.int32)
    groups = ops.adam_groups([dict(lr=1e-3, betas=(0.9, 0.99), eps=1e-8, weight_decay=0.0)] * 2)
    calls = (lambda **k: ops.adam_step_groups(BPM_BF16, torch.zeros(8, dtype=torch.uint8), 1, 1, f, f, f, f, groups, 1.0, False, **k),
             lambda **k: ops.adam_step_sets(BPM_BF16, (torch.zeros(8, dtype=torch.uint8), None, 1, 1),
                                            (torch.zeros(8, dtype=torch.uint8), (_lib.AdamSet * 1)(), None), groups, 1.0, False, **k))
    for call in calls:
        for key in ("scale_dev", "norm_dev"):
            for t in (torch.zeros(1, dtype=torch.float64), torch.zeros(0)):
                with pytest.raises(ValueError, match=key + ": expected float32"):
                    call(**{key: t})
        for t in (torch.zeros(2), i32(1), i32(4)[::2]):      # wrong dtype, fewer counters than groups, not contiguous
            with pytest.raises(ValueError, match="steps_dev.*int32 device counter"):
                call(steps_dev=t)
        for t in (torch.zeros(1), i32(0)):
            with pytest.raises(ValueError, match="skipped_dev: an int32 device counter"):
                call(skipped_dev=t)
        assert not rec.calls
        sc, nm, st, sk = torch.zeros(1), torch.zeros(1), i32(2), i32(1)
        call(scale_dev=sc, norm_dev=nm, steps_dev=st, skipped_dev=sk)
        (name, args), = rec.calls
        assert args[-6:-2] == (sc.data_ptr(), nm.data_ptr(), st.data_ptr(), sk.data_ptr()) and len(args) == len(_lib.SIGNATURES[name])
        rec.calls.clear()
