"""Head dims above 128 without a GPU: the padded-head_dim buckets, the launch tables of both models at head_dim 256 built
from host tensors (ops._DRY_RUN, as test_plan_tables_cpu.py) in both schedules, and the CPU oracle against the reference
fixtures F13 (mmtrvat, head_dim 256) and F14 (mmtrvapt, head_dim 192) of tests/golden/make_golden_wide_heads.py."""
from types import SimpleNamespace

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import engine, ops
from bpmult_amd.models import get_model
from detgen import det
from oracle import bpmult_cpu as O
from test_oracle_golden import _check_model, load, sd_for


def test_dhp_for_wide_heads():
    assert [engine.dhp_for(dh) for dh in (129, 136, 192, 256)] == [256] * 4
    assert [engine.dhp_for(dh) for dh in (25, 64, 128)] == [32, 64, 128]
    with pytest.raises(ValueError, match="256"):
        engine.dhp_for(257)


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    try:
        yield
    finally:
        ops._DRY_RUN = False


def _args(model, **kw):
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=512, vonly=True, lonly=True, aonly=True,
             num_heads=2, layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1, res_dropout=0.1,
             out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.mark.parametrize("prune", [True, False])
@pytest.mark.parametrize("model,kw", [("mmtrvat", {}), ("mmtrvat", {"hidden_sz": 384, "precision": "f32"}),
                                      ("mmtrvapt", {"orig_d_a": 96, "num_vectors_a": 40, "num_vectors_v": 40}),
                                      ("mmtrvapt", {"orig_d_a": 96, "hidden_sz": 272, "num_vectors_a": 40, "num_vectors_v": 40})])
def test_launch_tables_at_wide_heads(dry_run, model, kw, prune):
    """head_dim 256 / 192 / 136: every attention problem of both levels carries dhp 256; the pruned 3-modal level 2 takes
    the low-rank key side (no dK / dV pass, bpm_expand_heads instead)."""
    m = get_model(_args(model, prune_unused_rows=prune, **kw))
    m._ensure_store()
    trunk = m._trunk_for(2)
    assert trunk.prune == prune
    dh = m.hidden_sz // 2 if hasattr(m, "hidden_sz") else None
    un = lambda s: s[1] if isinstance(s, tuple) and s[0] in (engine.SIDE, engine.SIDE2) else s
    for plan in (trunk.plan1, trunk.plan2):
        assert plan.dhp == 256 and 128 < plan.dh <= 256 and (dh is None or plan.dh == dh)
        for training in (True, False):
            for first in (True, False):
                for s in plan._bwd[(training, first)]:
                    s = un(s)
                    if isinstance(s, tuple) and s[0] in (ops.attn_bwd_dq, ops.attn_bwd_dkv, ops.attn_bwd):
                        assert all(p.dhp == 256 and p.dh == plan.dh for p in s[2])
    if prune and model == "mmtrvat":
        assert trunk.plan2._lowrank
    for plan in (trunk.plan1, trunk.plan2):       # (level 1 qualifies too where T * H * 4 <= d)
        fns = [un(s)[0] for s in plan._bwd[(True, True)] if s is not engine.JOIN and isinstance(un(s), tuple)]
        assert (ops.attn_bwd_dkv not in fns) == plan._lowrank and (ops.expand_heads in fns) == plan._lowrank


def test_f13_wide_mmtrvat_oracle():
    g = load("f13_wide_mmtrvat")
    pfx = "f13."
    m = O.ModelCfg(512, 2, 2, 6, orig_d_l=32, num_vectors_l=64, num_vectors_a=64, num_vectors_v=64)
    shapes = O.model_param_shapes(m, False)
    ref = dict(zip(g["param_names"].tolist(), g["param_shapes"].tolist()))
    mine = {k: ",".join(map(str, v)) for k, v in shapes.items()}
    assert mine.keys() == ref.keys()
    # (the unused time-axis maps keep the reference's source-constant 512 x 512 shapes there: no gradient, see "nograd")
    assert {k: v for k, v in mine.items() if not k.startswith("transfm_")} == {k: v for k, v in ref.items() if not k.startswith("transfm_")}
    sd = sd_for(shapes, pfx)
    xl, img, aud = (torch.from_numpy(det(pfx + n, s)).requires_grad_(True) for n, s in
                    (("xl", (2, 20, 32)), ("img", (2, 60, 35)), ("aud", (2, 50, 74))))
    logits, z = O.bpmult3_forward(sd, m, xl, img, aud)
    _check_model(g, sd, logits, z, {"xl": xl, "img": img, "aud": aud}, pfx, tol=1e-5)


def test_f14_wide_mmtrvapt_oracle():
    g = load("f14_wide_mmtrvapt")
    pfx = "f14."
    m = O.ModelCfg(384, 2, 2, 13, orig_d_l=32, orig_d_v=40, orig_d_a=96, orig_d_p=64, num_vectors_a=200, num_vectors_v=200)
    shapes = O.model_param_shapes(m, True)
    assert {k: ",".join(map(str, v)) for k, v in shapes.items()} == dict(zip(g["param_names"].tolist(), g["param_shapes"].tolist()))
    sd = sd_for(shapes, pfx)
    xl, img, post = (torch.from_numpy(det(pfx + n, s)).requires_grad_(True) for n, s in
                     (("xl", (2, 60, 32)), ("img", (2, 150, 40)), ("post", (2, 64))))
    aud = torch.from_numpy(det(pfx + "aud", (2, 96, 1000)))
    logits, z = O.bpmult4_forward(sd, m, xl, img, O.audio_encoder(sd, aud), post)
    _check_model(g, sd, logits, z, {"xl": xl, "img": img, "post": post}, pfx, tol=1e-5)
