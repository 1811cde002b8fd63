"""Host logic without a GPU: the fused key / value source launches (bpm_kv_source_fwd / _bwd) in the launch tables.
Tables are built from HOST tensors (ops._DRY_RUN); nothing is launched.  Fused mode has no ke / ve / dke / dve buffers
and exactly one fused launch per direction and plan; a hidden size outside the kernels' domain and BPMULT_KV_FUSED=0
keep the embed_pos / LayerNorm launches; the trunk's gradient sums carry one term per key / value source, and the
pruned 3-modal trunk has no d(level-1 output) sum left.  Header, library exports and bindings agree."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, engine, ops
from bpmult_amd.models import get_model
from bpmult_amd.models.bpmult import LEVEL1, LEVEL2

ROOT = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
HEADER = open(os.path.join(ROOT, "include", "bpmult_hip.h")).read()


def _args(model, **kw):
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=64, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1, res_dropout=0.1,
             out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    try:
        yield
    finally:
        ops._DRY_RUN = False


def _un(s):
    return s[1] if isinstance(s, tuple) and s[0] in (engine.SIDE, engine.SIDE2) else s


def _launches(steps):
    return [_un(s) for s in steps if s is not engine.JOIN and callable(_un(s)[0])]


def _plan(d, H=2, L=2, B=2, T=5, S=7, n=2, embed_dropout=0.25):
    from bpmult_amd.models.encoder import TransformerEncoder
    encs = [TransformerEncoder(d, H, L, embed_dropout=embed_dropout, attn_mask=True) for _ in range(n)]
    st = engine.ParamStore([(f"e{j}.{k}", p) for j, m in enumerate(encs) for k, p in m.named_parameters()], _lib.BPM_BF16)
    for j in range(n):
        engine.register_encoder_shadows(st, f"e{j}.", d, L)
    st.finalize_shadows()
    cfg = engine.GroupCfg(d, H, L, 0.0, 0.0, embed_dropout, True, False)
    return engine.EncoderGroupPlan(st, cfg, [engine.EncoderDesc(f"e{j}.", j, T, S + j, 0.0) for j in range(n)], B)


def test_fused_tables(dry_run, monkeypatch):
    monkeypatch.delenv("BPMULT_KV_FUSED", raising=False)
    d, L, B = 24, 2, 2
    plan = _plan(d, L=L, B=B)
    assert plan._kv_fused
    for b in plan.buf:
        for k in ("ke", "ve", "dke", "dve"):
            assert k not in b, k
        assert b["khat"].shape == (b["Rk"], plan.ld) and b["dxk"].shape == b["dxv"].shape
    for training in (True, False):
        fwd = _launches(plan._fwd[training])
        fns = [s[0] for s in fwd]
        assert fns.count(ops.kv_source_fwd) == 1 and fns[0] is ops.kv_source_fwd     # ahead of the K / V projections
        assert fns.count(ops.ln_fwd) == 2 * L + 1                                       # LayerNorm-0, FFN, final: no hat launch
        assert plan._fwd[training][0][0] is engine.SIDE and plan._fwd[training][1] == (engine.MARK, "hat")
        arr = fwd[0][2]
        assert len(arr) == len(plan.encs) and fwd[0][3] is plan.table and fwd[0][4] == d
        for p, e, b in zip(arr, plan.encs, plan.buf):
            assert (p.T, p.B, p.ld) == (e.S, B, plan.ld) and p.khat == b["khat"].data_ptr() and p.vhat == b["vhat"].data_ptr()
            assert p.gk == b["Gk"].data_ptr() and p.gv == b["Gv"].data_ptr()
            assert p.dxk == b["dxk"].data_ptr() and p.dxv == b["dxv"].data_ptr()          # separate gradients by default
            assert p.drop_site_k != p.drop_site_v and p.drop_p_k == p.drop_p_v == pytest.approx(0.25 if training else 0.0)
            assert p.mean_k == b["stk"][0].data_ptr() and p.rstd_v == b["stv"][1].data_ptr()
        for stores in (True, False):
            steps = plan._bwd[(training, stores)]
            bwd = _launches(steps)
            fns = [s[0] for s in bwd]
            assert fns.count(ops.kv_source_bwd) == 1 and fns[-1] is ops.kv_source_bwd
            assert steps[-1] is engine.JOIN and steps[-2][0] is engine.SIDE
            assert bwd[-1][1] is arr                                                     # one problem array for both directions
            assert all(len(s[1]) == len(plan.encs) for s in bwd if s[0] is ops.ln_bwd)   # no hat problems among them
    dq, dk, dv = plan.input_grads()
    assert all(a is b["dxk"] for a, b in zip(dk, plan.buf)) and all(a is b["dxv"] for a, b in zip(dv, plan.buf))


def test_merge_kv_grads(dry_run, monkeypatch):
    monkeypatch.delenv("BPMULT_KV_FUSED", raising=False)
    plan = _plan(24)
    dst = torch.zeros(plan.encs[1].S, 2, 24)
    assert plan.merge_kv_grads([None, dst]) is True
    dq, dk, dv = plan.input_grads()
    assert dk[0] is plan.buf[0]["dxk"] and dk[1] is dst and dv == [None, None]
    for arr in plan._kvsrc.values():
        assert arr[0].dxk == plan.buf[0]["dxk"].data_ptr() and arr[1].dxk == dst.data_ptr()
        assert arr[0].dxv is None and arr[1].dxv is None
    with pytest.raises(ValueError):
        plan.merge_kv_grads([None, torch.zeros(3, 2, 24)])


@pytest.mark.parametrize("how", ["hidden 50", "BPMULT_KV_FUSED=0"])
def test_old_route(dry_run, monkeypatch, how):
    if how == "hidden 50":
        monkeypatch.delenv("BPMULT_KV_FUSED", raising=False)
        d = 50
    else:
        monkeypatch.setenv("BPMULT_KV_FUSED", "0")
        d = 24
    L = 2
    plan = _plan(d, L=L)
    assert not plan._kv_fused and plan._kvsrc == {}
    for b in plan.buf:
        for k in ("ke", "ve", "dke", "dve"):
            assert b[k].shape == (b["Rk"], d)
    fwd = _launches(plan._fwd[True])
    fns = [s[0] for s in fwd]
    assert ops.kv_source_fwd not in fns and fns[0] is ops.ln_fwd and fns.count(ops.ln_fwd) == 2 * L + 2
    assert len(fwd[0][2]) == 2 * len(plan.encs) and fwd[0][2][0].x == plan.buf[0]["ke"].data_ptr()
    bwd = _launches(plan._bwd[(True, True)])
    assert ops.kv_source_bwd not in [s[0] for s in bwd] and bwd[-1][0] is ops.ln_bwd
    assert bwd[-1][1][1].dx == plan.buf[0]["dve"].data_ptr()
    assert plan.merge_kv_grads() is False                                   # nothing to merge with: two gradients as before
    dq, dk, dv = plan.input_grads()
    assert all(a is b["dxk"] for a, b in zip(dk, plan.buf)) and all(a is b["dxv"] for a, b in zip(dv, plan.buf))


def _ptrs(p):
    return [p.src[j] for j in range(p.n_in)]


@pytest.mark.parametrize("prune", [True, False])
def test_trunk_sums_carry_one_term_per_source(dry_run, monkeypatch, prune):
    monkeypatch.delenv("BPMULT_KV_FUSED", raising=False)
    m = get_model(_args("mmtrvat", prune_unused_rows=prune))
    m._ensure_store()
    trunk = m._trunk_for(2)
    p1, p2 = trunk.plan1, trunk.plan2
    assert p1._kv_fused and p2._kv_fused
    dq1, dk1, dv1 = p1.input_grads()
    dq2, dk2, dv2 = p2.input_grads()
    assert dv1 == [None] * 6 and dv2 == [None] * 6
    assert all(g is b["dxk"] for g, b in zip(dk1, p1.buf))
    if prune:
        # the merged level-2 gradient is the only whole-tensor term of d(level-1 output): written in place, no sum launch
        assert len(trunk._sum_d1) == 0
        for (n, (q, src, _)), g in zip(LEVEL2.items(), dk2):
            assert g is trunk.d1buf[src]
        for arr in p2._kvsrc.values():
            assert [p.dxk for p in arr] == [trunk.d1buf[src].data_ptr() for (q, src, _) in LEVEL2.values()]
    else:
        assert len(trunk._sum_d1) == 6
        for p, g, b in zip(trunk._sum_d1, dk2, p2.buf):
            assert g is b["dxk"] and p.n_in == 3 and _ptrs(p)[-1] == g.data_ptr()      # two GMU terms + ONE key / value term
    # d(projected input): per modality its query gradients and one term per encoder that reads it as key / value source
    by_dst = {p.out: p for p in trunk._sum_dpx}
    for k in ("l", "a", "v"):
        p = by_dst[trunk.dpx[k].data_ptr()]
        kv_terms = [g.data_ptr() for (n, (q, kv, _)), g in zip(LEVEL1.items(), dk1) if kv == k]
        assert len(kv_terms) == 2 and all(t in _ptrs(p) for t in kv_terms)
        n_q = sum(q == k for (q, kv, _) in LEVEL1.values()) + (0 if prune else sum(q == k for (q, s, _) in LEVEL2.values()))
        assert p.n_in == n_q + 2


def test_trunk_keeps_two_terms_without_the_fused_launch(dry_run, monkeypatch):
    monkeypatch.setenv("BPMULT_KV_FUSED", "0")
    m = get_model(_args("mmtrvat", prune_unused_rows=True))
    m._ensure_store()
    trunk = m._trunk_for(2)
    assert not trunk.plan1._kv_fused and len(trunk._sum_d1) == 6
    assert all(p.n_in == 2 for p in trunk._sum_d1)
    assert all(g is not None for g in trunk.plan2.input_grads()[2])


def test_header_exports_and_bindings_agree():
    lib = _lib.lib()
    for name in ("bpm_kv_source_fwd", "bpm_kv_source_bwd"):
        assert re.search(r"^int %s\(" % name, HEADER, flags=re.M), name
        assert hasattr(lib, name) and name in _lib.SIGNATURES
    body = re.search(r"typedef struct bpm_kv_source_problem \{(.*?)\} bpm_kv_source_problem;", HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        parts = decl.strip().split(",")
        if parts[0]:
            names.append(parts[0].split()[-1].lstrip("*"))
            names += [p.strip().lstrip("*") for p in parts[1:]]
    assert names == [f[0] for f in _lib.KvSourceProblem._fields_]
    # argument counts of the declarations and of the bindings
    for name in ("bpm_kv_source_fwd", "bpm_kv_source_bwd"):
        decl = re.search(r"^int %s\((.*?)\);" % name, HEADER, flags=re.M | re.S).group(1)
        assert len(decl.split(",")) == len(_lib.SIGNATURES[name]), name
    # the domain is enforced before anything is launched: no device is needed to be refused
    p = _lib.KvSourceProblem()
    assert lib.bpm_kv_source_fwd(_lib.BPM_BF16, C.byref(p), 1, None, 0, 24, 1.0, 1e-5, 0, None) == -1
    assert lib.bpm_kv_source_bwd(C.byref(p), 1, None, 0, 24, 1.0, 0, None) == -1
    assert lib.bpm_kv_source_bwd(None, 1, None, 0, 24, 1.0, 0, None) == -1
    assert ops.kv_source_ok(24, 7, 2) and ops.kv_source_ok(1024, 512, 8)
    assert not ops.kv_source_ok(50, 7, 2) and not ops.kv_source_ok(1028, 7, 2) and not ops.kv_source_ok(768, 1 << 20, 8)
