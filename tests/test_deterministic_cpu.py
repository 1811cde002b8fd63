"""Deterministic mode without a GPU: the switch, and the launch tables it builds (ops._DRY_RUN, as
tests/test_plan_tables_cpu.py does).  In deterministic mode no step of a backward table may add floats in hardware
order: no GemmProblem / CastProblem / LnProblem carries a column-sum pointer that an atomics epilogue or row kernel
would serve, every fc1 / fc2 / out_proj weight-gradient product carries that layer's bias gradient as colsum_a, every
LayerNorm backward is marked for bpm_ln_bwd_det (ops.ln_det) and every unfold through bpm_unfold_grads_ws.  In default mode the
tables are the parent commit's (digest of tools/plan_digest.py, profiles/plan_digest_default.json)."""
import hashlib
import importlib
import json
import os
import sys
from types import SimpleNamespace

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import config, engine, ops
from bpmult_amd._lib import GEMM_TN
from bpmult_amd.models import get_model
from bpmult_amd.models.attention import MultiheadAttention
from bpmult_amd.models.encoder import TransformerEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _args(model, **kw):
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=64, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1, res_dropout=0.1,
             out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


MODELS = [("mmtrvat", {}), ("mmtrvat", {"hidden_sz": 40, "precision": "f32"}),
          ("mmtrvapt", {"orig_d_a": 96, "num_vectors_a": 40, "num_vectors_v": 40}),
          ("mmtrvapt", {"orig_d_a": 96, "hidden_sz": 40, "num_vectors_a": 40, "num_vectors_v": 40})]


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    try:
        yield
    finally:
        ops._DRY_RUN = False


@pytest.fixture
def restore_config():
    det, prec = config.deterministic(), config.precision()
    try:
        yield
    finally:
        config.set_deterministic(det)
        config.set_precision(prec)


def test_switch_round_trips(dry_run, restore_config, monkeypatch):
    """config, the environment variable, args, model.set_deterministic (which drops the trunks) and the modules' attribute."""
    config.set_deterministic(True)
    assert config.deterministic() is True
    config.set_deterministic(False)
    assert config.deterministic() is False
    for value, want in (("1", True), ("0", False), (None, False)):       # read at import, the way BPMULT_PRECISION is
        if value is None:
            monkeypatch.delenv("BPMULT_DETERMINISTIC", raising=False)
        else:
            monkeypatch.setenv("BPMULT_DETERMINISTIC", value)
        importlib.reload(config)
        assert config.deterministic() is want
    # args: None means the process default, read when the tables are built
    m = get_model(_args("mmtrvat"))
    assert m.deterministic is None and m.enc.deterministic is None
    t = m._trunk_for(2)
    assert t.det is False and t.plan1.det is False and t.plan2.det is False
    config.set_deterministic(True)
    assert m._trunk_for(2) is t and t.plan1.det is False       # the built tables keep the mode they were built in
    m.set_prune_unused_rows(m.prune_unused_rows)                # (anything that drops the trunks: the next ones read the default)
    assert m._trunk_for(2).plan1.det is True
    config.set_deterministic(False)
    m = get_model(_args("mmtrvat", deterministic=True))
    assert m.deterministic is True and m.enc.deterministic is True
    t = m._trunk_for(2)
    assert t.det and t.plan1.det and t.plan2.det
    m.set_deterministic(False)
    assert m._trunks == {} and m.deterministic is False and m.enc.deterministic is False
    assert m._trunk_for(2).plan2.det is False
    m.set_deterministic(None)
    assert m._trunks == {} and m.deterministic is None
    # the stand-alone modules: an attribute, None meaning the config value
    enc = TransformerEncoder(24, 4, 2)
    assert enc.deterministic is None and MultiheadAttention(24, 4).deterministic is None
    x = torch.zeros(5, 2, 24)
    assert enc._plan_for(x, x).det is False
    enc.deterministic = True
    assert enc._plan_for(x, x).det is True and enc._plan_for(x, None).det is True
    enc.deterministic = None
    assert enc._plan_for(x, x).det is False


def _steps(table):
    for s in table:
        if s is engine.JOIN or s[0] in (engine.MARK, engine.WAIT):
            continue
        yield s[1] if s[0] in (engine.SIDE, engine.SIDE2) else s


def _bias_owners(plan):
    """{address of a weight gradient: address of its layer's bias gradient} for fc1 / fc2 / out_proj of every encoder and layer."""
    st, own = plan.store, {}
    for e in plan.encs:
        for i in range(plan.cfg.layers):
            for leaf in ("fc1", "fc2", "self_attn.out_proj"):
                own[st.gptr(plan._pn(e, i, leaf + ".weight"))] = st.gptr(plan._pn(e, i, leaf + ".bias"))
    return own


def _walk(plan, det):
    """The structural checks of one plan's four backward tables; det False: what the default tables hold instead."""
    assert plan.det is det
    own = _bias_owners(plan)
    for key, table in plan._bwd.items():
        seen = {w: 0 for w in own}
        n_ln = n_unfold = 0
        for s in _steps(table):
            fn = s[0]
            assert fn is not (ops.unfold_grads if det else ops.unfold_grads_ws), key
            if fn is ops.gemm_grouped:
                for q in s[3]:
                    if det:
                        assert not q.colsum, key                  # the epilogue's column sums are float atomics
                    if s[2] == GEMM_TN and q.C in own:
                        seen[q.C] += 1
                        assert q.colsum_a == (own[q.C] if det else None), key
                    elif det:
                        assert q.colsum_a not in own.values(), key
            elif fn is ops.rows_cast:
                assert not det or all(not q.colsum for q in s[2]), key
            elif fn is ops.ln_bwd:
                n_ln += 1
                assert getattr(s[1], "det", False) is det, key           # -> bpm_ln_bwd_det: atomics are an error there
                assert not det or all(not q.cast_colsum for q in s[1]), key
            elif fn in (ops.unfold_grads, ops.unfold_grads_ws):
                n_unfold += 1
                if det:
                    assert s[4] == plan.cfg.d                   # max_cols: every descriptor is [2d, d]
        assert all(n >= 1 for n in seen.values()), key
        assert n_ln >= plan.cfg.layers and n_unfold == (plan.cfg.layers if plan._kv else 0), key


@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("model,kw", MODELS)
def test_deterministic_tables_have_no_atomic_sums(dry_run, model, kw, prune):
    m = get_model(_args(model, prune_unused_rows=prune, deterministic=True, **kw))
    trunk = m._trunk_for(2)
    for plan in (trunk.plan1, trunk.plan2):
        assert set(plan._bwd) == {(t, f) for t in (True, False) for f in (True, False)}     # training x stores
        _walk(plan, True)
    m.set_deterministic(False)                   # the same model in default mode: the sums are where they always were
    trunk = m._trunk_for(2)
    for plan in (trunk.plan1, trunk.plan2):
        _walk(plan, False)
        assert any(q.colsum for s in _steps(plan._bwd[(True, True)]) if s[0] is ops.gemm_grouped for q in s[3])


@pytest.mark.parametrize("bi", [False, True])
@pytest.mark.parametrize("form", ["self", "cross"])
def test_stand_alone_encoder_plan(dry_run, bi, form):
    enc = TransformerEncoder(24, 4, 2, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.1, attn_mask=True,
                             biprojection=bi)
    enc.deterministic = True
    x = torch.zeros(7, 2, 24)
    _walk(enc._plan_for(x, None if form == "self" else x), True)


def test_step_functions_registered():
    assert ops.ln_det([ops.ln_problem(None, None, None, None, None, 1)]).det is True
    assert ops.unfold_grads_ws in ops.STEP_FUNCTIONS and ops.unfold_grads_ws not in ops.SEEDED


# ---- the drivers that launch directly (no step table): models/attention.py and models/bert.py ---------------------
class Recorder:
    """Stands in for the loaded library (as tests/test_ops_launch_cpu.py's): size queries answered, every other bpm_*
    entry records (name, args) and returns 0."""
    def __init__(self):
        self.calls = []

    def __getattr__(self, name):
        if not name.startswith("bpm_"):
            raise AttributeError(name)
        if name.endswith("_bytes"):
            return lambda *a: 1 << 10
        return lambda *a: self.calls.append((name, a, self._copy(a))) or 0

    @staticmethod
    def _copy(args):
        """The problem structs of a grouped call, copied while the caller's array is alive (pointer, then its count)."""
        import ctypes as C
        for k, a in enumerate(args):
            if isinstance(a, C._Pointer):
                n = next(x for x in args[k + 1:] if isinstance(x, int))
                return [type(a.contents).from_buffer_copy(bytes(memoryview(a[i]))) for i in range(n)]
        return []


@pytest.fixture
def rec(monkeypatch):
    from bpmult_amd import _lib
    r = Recorder()
    monkeypatch.setattr(_lib, "_lib", r)
    monkeypatch.setattr(ops, "_stream", lambda: 0)
    monkeypatch.setattr(ops, "_DRY_RUN", True)
    ws = torch.zeros(1 << 8)
    monkeypatch.setattr(ops, "_ln_workspace", lambda n, d, device, *entry: ws)
    monkeypatch.setattr(torch.cuda, "current_device", lambda: 0)
    return r


def _problems(call):
    return call[2]


def _no_atomic_sums(calls, det):
    """No recorded call reaches an entry or carries a pointer that adds with float atomics (deterministic mode); the
    names of the entries that were called."""
    names = [c[0] for c in calls]
    for c in calls:
        if c[0] == "bpm_gemm_grouped":
            assert not det or all(not q.colsum and q.splitk <= 1 for q in _problems(c))
        if c[0] == "bpm_rows_cast":
            assert not det or all(not q.colsum for q in _problems(c))
        if c[0] in ("bpm_ln_bwd_ws", "bpm_ln_bwd_det"):
            assert not det or all(not q.cast_colsum for q in _problems(c))
    if det:
        assert "bpm_ln_bwd_ws" not in names and "bpm_ln_bwd" not in names and "bpm_unfold_grads" not in names
    return names


@pytest.mark.parametrize("det", [True, False])
def test_multihead_attention_backward_launches(rec, det):
    from bpmult_amd.models.attention import _Exec
    from bpmult_amd._lib import GEMM_TN
    d, T, B = 32, 5, 2
    m = MultiheadAttention(d, 4)
    ex = _Exec(m, torch.device("cpu"), "f32", det)
    pl = ex.plan(T, T, B, "qkv")
    rec.calls.clear()
    grads = ex.backward(m, pl, torch.zeros(T, B, d))[4]
    _no_atomic_sums(rec.calls, det)
    g_ob = grads[3].data_ptr()
    tn = [q for c in rec.calls if c[0] == "bpm_gemm_grouped" and c[1][1] == GEMM_TN for q in _problems(c)]
    ride = [q for q in tn if q.colsum_a == g_ob]
    cast = [q for c in rec.calls if c[0] == "bpm_rows_cast" for q in _problems(c) if q.colsum == g_ob]
    assert (len(ride), len(cast)) == ((1, 0) if det else (0, 1))
    assert not det or ride[0].C == grads[2].data_ptr()                 # on the out_proj weight-gradient product


@pytest.mark.parametrize("det", [True, False])
def test_bert_stack_backward_launches(rec, det):
    from transformers import BertConfig, BertModel
    from bpmult_amd._lib import GEMM_TN
    from bpmult_amd.models.bert import LAYER_PARAMS, BertLayerStack
    bert = BertModel(BertConfig(vocab_size=30, hidden_size=64, num_attention_heads=2, num_hidden_layers=2, intermediate_size=128,
                                max_position_embeddings=16))
    st = BertLayerStack(bert, "f32")
    st.deterministic = det
    B, L = 2, 7
    st.forward(torch.zeros(B, L, 64), torch.ones(B, L, dtype=torch.uint8), 5, True)
    pl = st._plan(B, L)
    assert pl.det is det
    rec.calls.clear()
    _, grads = st.backward(pl, torch.zeros(B, L, 64), True)
    names = _no_atomic_sums(rec.calls, det)
    assert names.count("bpm_ln_bwd_det" if det else "bpm_ln_bwd_ws") == 2 * 2
    G = lambda i, n: grads[i * len(LAYER_PARAMS) + LAYER_PARAMS.index(n)].data_ptr()
    tn = {q.C: q for c in rec.calls if c[0] == "bpm_gemm_grouped" and c[1][1] == GEMM_TN for q in _problems(c)}
    ln = [q for c in rec.calls if c[0].startswith("bpm_ln_bwd") for q in _problems(c)]
    for i in range(2):
        for leaf in ("output.dense", "attention.output.dense"):
            bias = G(i, leaf + ".bias")
            assert tn[G(i, leaf + ".weight")].colsum_a == (bias if det else None)
            assert sum(q.cast_colsum == bias for q in ln) == (0 if det else 1)
        for leaf in ("intermediate.dense", "attention.self.query", "attention.self.key", "attention.self.value"):
            assert tn[G(i, leaf + ".weight")].colsum_a == G(i, leaf + ".bias")      # these ride in both modes


# ---- the new row entries: dry dispatch of the -DBPM_LAB build ------------------------------------------------------
@pytest.fixture(scope="module")
def lab():
    from bpmult_amd import _lib
    _lib.build_lab()
    with _lib.lab_library() as L:
        yield L


def _dispatch_record():
    with open(os.path.join(ROOT, "profiles", "deterministic_dispatch.json")) as f:
        return json.load(f)


def test_dispatch_record_covers_the_case_table():
    import deterministic_cases
    assert list(_dispatch_record()) == list(deterministic_cases.CASES)


def test_new_row_entries_launch_what_is_recorded(lab):
    import deterministic_cases
    import rowops_cases
    record = _dispatch_record()
    for name, fn in deterministic_cases.CASES.items():
        assert rowops_cases.run(lab, fn) == record[name], name


def test_every_refusal_stands_beside_an_accepted_call():
    """What the record must show, whatever produced it: the scalar family and shared rows are COMPUTED (two launches, no
    kernel that adds with atomics), the vector route is bpm_ln_bwd_ws's, and a call is refused only for its workspace."""
    rec_ = _dispatch_record()
    kernels = lambda name: [l[0].split("<")[0] for l in rec_[name]["launches"]]
    for dt in ("f32", "bf16"):
        for d in (24, 256, 768, 1024):
            assert rec_[f"ln_bwd_det {dt} d={d}"]["rc"] == 0 and kernels(f"ln_bwd_det {dt} d={d}") == ["ln_bwd_vec_kernel"]
        for what in ("d=50", "d=770", "d=1028", "d=1536", "d=2048", "d=768 shared dgamma", "d=768 dbeta 4 bytes off", "d=768 x 4 bytes off"):
            assert rec_[f"ln_bwd_det {dt} {what}"]["rc"] == 0, what
            assert kernels(f"ln_bwd_det {dt} {what}") == ["ln_bwd_part_kernel", "col_finish_kernel"], what
        assert rec_[f"ln_bwd_det {dt} d=2049"] == {"rc": -1, "launches": []}              # past every kernel's reach, as in bpm_ln_bwd
        assert kernels(f"ln_bwd_det {dt} d=50 no sums at all, no workspace") == ["ln_bwd_kernel"]
        for d in (50, 768):
            for why in ("null workspace", "workspace one float short"):
                assert rec_[f"ln_bwd_det {dt} d={d} {why}"] == {"rc": -1, "launches": []}
        assert kernels(f"rows_cast_ws {dt} sums only 129x36") == ["colsum_part_kernel", "col_finish_kernel"]
        for what in ("sums only 129x37", "sums only 129x1028", "sums only 33x36, a 4 bytes off", "sums only 33x36 beside 33x37",
                     "dst_ct 33x36 and 129x1028", "shared colsum"):
            assert kernels(f"rows_cast_ws {dt} {what}") == ["rows_cast_part_kernel", "col_finish_kernel"], what
        assert kernels(f"rows_cast_ws {dt} dst_ct, no sums") == ["rows_cast_kernel"]
        for why in ("null workspace", "workspace short"):
            assert rec_[f"rows_cast_ws {dt} {why}"] == {"rc": -1, "launches": []}
    assert all(k not in ("ln_bwd_kernel", "rows_cast_kernel", "colsum_kernel", "unfold_grads_kernel") or "no sums" in name
               for name in rec_ for k in kernels(name))
    assert kernels("unfold_grads_ws 37 columns") == ["unfold_grads_ws_kernel"]


def default_mode_digests():
    """{label: SHA-256 of tools/plan_digest.py's canonical JSON of one plan} for this file's models in both schedules
    and three precisions, and a stand-alone encoder of each layer kind.  (tools/plan_digest.py's own main() walks 384
    trunks and prints 200 MB: the whole of it was compared once, see profiles/plan_digest_default.json.)"""
    sys.path.insert(0, os.path.join(ROOT, "tools"))
    try:
        import plan_digest
    finally:
        sys.path.pop(0)
    sha = lambda plan: hashlib.sha256(json.dumps(plan_digest.digest(plan), sort_keys=True, separators=(",", ":")).encode()).hexdigest()
    out = {}
    for (model, kw), prune, prec in [(mk, p, q) for mk in MODELS for p in (True, False) for q in ("bf16", "f32", "bf16x3")]:
        m = get_model(_args(model, prune_unused_rows=prune, **{**kw, "precision": prec}))
        trunk = m._trunk_for(2)
        for k, plan in (("plan1", trunk.plan1), ("plan2", trunk.plan2)):
            out[f"{model} {sorted(kw.items())} prune={prune} {prec} {k}"] = sha(plan)
    for bi in (False, True):
        enc = TransformerEncoder(24, 4, 2, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.1, attn_mask=True,
                                 biprojection=bi)
        x = torch.zeros(7, 2, 24)
        for form, xk in (("self", None), ("cross", x)):
            out[f"encoder bi={bi} {form}"] = sha(enc._plan_for(x, xk))
    return out


def test_default_tables_equal_the_parent_commits(dry_run, restore_config):
    """Default mode: every step, every field of every problem struct, every pointer (as allocation number and offset) of the
    launch tables is what the parent commit built -- the digests recorded from it in profiles/plan_digest_default.json."""
    config.set_deterministic(False)
    with open(os.path.join(ROOT, "profiles", "plan_digest_default.json")) as f:
        want = json.load(f)["plans"]
    got = default_mode_digests()
    assert set(got) == set(want) and len(got) == 52
    assert [k for k in got if got[k] != want[k]] == []
