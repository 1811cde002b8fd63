"""Host logic without a GPU: the self-attention-only encoder plan (TransformerEncoder.forward(x); engine GroupCfg.self_only)
builds its forward and backward launch tables from HOST tensors (ops._DRY_RUN) for both layer kinds and all three
precisions.  Nothing is launched; the checks are structural: no key / value-side state or steps, one storing first
writer per large weight-gradient block, and the FFN LayerNorm of the biprojection kind is layer_norms.2."""
import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import engine, ops
from bpmult_amd._lib import F_ACCUM, GEMM_TN
from bpmult_amd.models.encoder import TransformerEncoder


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


@pytest.mark.parametrize("prec", ["bf16", "f32", "bf16x3"])
@pytest.mark.parametrize("bi,d,H,L,Tn", [(False, 24, 4, 2, 9), (True, 24, 4, 2, 7), (False, 50, 2, 3, 70), (True, 512, 2, 1, 40)])
def test_self_only_tables(dry_run, prec, bi, d, H, L, Tn):
    B = 2
    enc = TransformerEncoder(d, H, L, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.1, attn_mask=True,
                             biprojection=bi)
    enc.precision = prec
    st = enc._ensure_store()
    x = torch.zeros(Tn, B, d)
    plan = enc._plan_for(x, None)
    assert plan.cfg.self_only and plan.cfg.biprojection == bi and not plan._lowrank and plan._unfold == []
    assert enc._plan_for(x, x) is not plan and not enc._plan_for(x, x).cfg.self_only      # keyed by call form
    (b,) = plan.buf
    for k in ("ke", "ve", "khat", "vhat", "dkall", "dvall", "dWf", "dbf", "Gk", "Gv", "dSall", "qs", "dke", "dxk"):
        assert k not in b, k
    assert b["dqkvs"][0].shape == (Tn * B + 1, 3 * plan.ld)
    ln_w = {i: {n: st.p(f"layers.{i}.layer_norms.{n}.weight").data_ptr() for n in range(3 if bi else 2)} for i in range(L)}
    g_w = {i: {n: st.gptr(f"layers.{i}.layer_norms.{n}.weight") for n in range(3 if bi else 2)} for i in range(L)}
    lnF = 2 if bi else 1
    for training in (True, False):
        fwd = _launches(plan._fwd[training])
        fns = [s[0] for s in fwd]
        assert fns.count(ops.attn_fwd) == L and ops.rows_cast not in fns
        assert fns.count(ops.ln_fwd) == 2 * L + 1 and fns.count(ops.gemm_grouped) == 4 * L
        attn = [p for s in fwd if s[0] is ops.attn_fwd for p in s[2]]
        assert all(p.T == p.S == Tn and p.mask_off == 1 for p in attn)
        # LayerNorm-0, then the FFN LayerNorm of every layer, then the final one
        lns = [s[2][0] for s in fwd if s[0] is ops.ln_fwd]
        for i in range(L):
            assert lns[2 * i].gamma == ln_w[i][0] and lns[2 * i + 1].gamma == ln_w[i][lnF]
        for stores in (True, False):
            bwd = _launches(plan._bwd[(training, stores)])
            fns = [s[0] for s in bwd]
            assert ops.unfold_grads not in fns and ops.attn_bwd_dq not in fns and ops.attn_bwd_dkv not in fns
            assert ops.expand_heads not in fns and fns.count(ops.attn_bwd) == L
            lnb = [p for s in bwd if s[0] is ops.ln_bwd for p in s[1]]
            assert len(lnb) == 2 * L
            for i in range(L):
                dg = {p.dgamma for p in lnb}
                assert g_w[i][0] in dg and g_w[i][lnF] in dg
                if bi:
                    assert g_w[i][1] not in dg                 # layer_norms.1: no gradient in the biprojection kind
            # large weight-gradient blocks: exactly one first writer each, storing iff stores
            first = {}
            for s in bwd:
                if s[0] is ops.gemm_grouped and s[2] == GEMM_TN:
                    for p in s[3]:
                        first.setdefault(p.C, []).append(not (p.flags & F_ACCUM))
            blocks = {st.gptr(f"layers.{i}.{leaf}") for i in range(L) for leaf in
                      ("self_attn.out_proj.weight", "fc1.weight", "fc2.weight")}
            blocks |= {st.gptr(f"layers.{i}.self_attn.in_proj_weight", w * d * d) for i in range(L) for w in range(3)}
            assert set(first) == blocks
            assert all(v == [stores] for v in first.values()), first
        acc, sto = plan._bwd[(training, False)], plan._bwd[(training, True)]
        assert len(acc) == len(sto)


def test_group_of_three_self_only(dry_run):
    """Three self-only encoders in lock-step: every launch of a layer serves all of them."""
    d, H, L, B = 24, 4, 2, 2
    encs = [TransformerEncoder(d, H, L, attn_mask=True) for _ in range(3)]
    named = [(f"e{j}.{k}", p) for j, m in enumerate(encs) for k, p in m.named_parameters()]
    st = engine.ParamStore(named, ops._lib.BPM_BF16)
    for j in range(3):
        engine.register_encoder_shadows(st, f"e{j}.", d, L)
    st.finalize_shadows()
    cfg = engine.GroupCfg(d, H, L, 0.0, 0.0, 0.0, True, False, self_only=True)
    plan = engine.EncoderGroupPlan(st, cfg, [engine.EncoderDesc(f"e{j}.", j, Tn, Tn, 0.0) for j, Tn in enumerate((5, 9, 6))], B)
    for s in _launches(plan._fwd[True]) + _launches(plan._bwd[(True, True)]):
        if s[0] is ops.gemm_grouped:
            assert len(s[3]) % 3 == 0
        elif s[0] in (ops.ln_fwd, ops.ln_bwd, ops.attn_fwd, ops.attn_bwd):
            assert len(s[2] if s[0] in (ops.ln_fwd, ops.attn_fwd, ops.attn_bwd) else s[1]) == 3
    with pytest.raises(ValueError):
        engine.EncoderGroupPlan(st, cfg, [engine.EncoderDesc("e0.", 0, 5, 7, 0.0)], B)


def test_default_group_cfg_is_not_self_only():
    cfg = engine.GroupCfg(24, 4, 2, 0.0, 0.0, 0.0, True, False)
    assert cfg.self_only is False
    assert TransformerEncoder(24, 4, 2).group_cfg().self_only is False
