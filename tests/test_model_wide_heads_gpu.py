"""Whole models and the standalone encoder at head_dim above 128 on the MI355X: the reference fixtures F13 (mmtrvat,
d=512 / 2 heads: head_dim 256) and F14 (mmtrvapt, d=384 / 2 heads: head_dim 192, zero-padded to 256) in every precision
and both schedules, the TransformerEncoder at head_dim 256 against the CPU oracle, the low-rank key side against the
dK / dV route, and graph replay against eager launches.  Limits: those of test_model_gpu.py / test_encoder_gpu.py."""
import copy

import pytest
import torch

pytestmark = pytest.mark.gpu

from detgen import det, det_param  # noqa: E402

import bpmult_amd  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.models.encoder import TransformerEncoder  # noqa: E402
from oracle import bpmult_cpu as O  # noqa: E402
from test_model_gpu import SCHEDULES, _record, args_for, load, run_model  # noqa: E402

T = torch.from_numpy


@pytest.mark.parametrize("prune", SCHEDULES)
@pytest.mark.parametrize("prec", ["f32", "bf16", "bf16x3"])
def test_f13_wide_mmtrvat(prec, prune):
    g = load("f13_wide_mmtrvat")
    model = get_model(args_for("mmtrvat", hidden_sz=512, num_heads=2, layers=2, orig_d_l=32, num_vectors_l=64, num_vectors_a=64,
                               num_vectors_v=64))
    assert sorted(k for k, _ in model.named_parameters()) == sorted(g["param_names"].tolist())
    inputs = {"xl": T(det("f13.xl", (2, 20, 32))), "img": T(det("f13.img", (2, 60, 35))), "aud": T(det("f13.aud", (2, 50, 74)))}
    run_model(g, model, "f13.", inputs, lambda m, d: m(d["xl"], None, None, d["img"], d["aud"], output_gate=True), prec,
              prune=prune)


@pytest.mark.parametrize("prune", SCHEDULES)
@pytest.mark.parametrize("prec", ["f32", "bf16", "bf16x3"])
def test_f14_wide_mmtrvapt(prec, prune):
    g = load("f14_wide_mmtrvapt")
    model = get_model(args_for("mmtrvapt", hidden_sz=384, num_heads=2, layers=2, orig_d_l=32, orig_d_v=40, orig_d_a=96,
                               orig_d_p=64, n_classes=13))
    assert sorted(k for k, _ in model.named_parameters()) == sorted(g["param_names"].tolist())
    inputs = {"xl": T(det("f14.xl", (2, 60, 32))), "img": T(det("f14.img", (2, 150, 40))),
              "aud": T(det("f14.aud", (2, 96, 1000))), "post": T(det("f14.post", (2, 64)))}
    run_model(g, model, "f14.", inputs,
              lambda m, d: m(d["xl"], None, None, d["img"], d["aud"], d["post"], output_gate=True), prec, prune=prune)


def _rel(a, b):
    a, b = a.detach().double().cpu(), b.detach().double().cpu()
    return float((a - b).norm() / max(float(b.norm()), 1e-12))


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("bi,mask", [(False, True), (False, False), (True, True), (True, False)])
def test_encoder_head_dim_256_against_oracle(prec, bi, mask):
    """TransformerEncoder d=512, 2 heads (head_dim 256), 2 layers, T=70 / S=100, crossmodal or biprojection: output and
    every gradient against oracle.encoder (fp32 CPU).  f32: 2e-4 of the tensor's max (test_encoder_gpu.py); bf16: the
    relative-L2 limits of test_encoder_gpu.py (y 1e-2, input gradients 1e-1, weights 1.4e-1, LayerNorm affines 2e-1)."""
    d, H, Ly, B, Tn, S = 512, 2, 2, 2, 70, 100
    pfx = f"wide_enc{int(bi)}{int(mask)}."
    enc = TransformerEncoder(d, H, Ly, attn_mask=mask, biprojection=bi)
    enc.precision = prec
    sd = {}
    with torch.no_grad():
        for k, p in enc.named_parameters():
            v = T(det_param(pfx + k, p.shape))
            p.copy_(v)
            sd[k] = v.clone().requires_grad_(True)
    x0, kv0 = T(det(pfx + "x", (Tn, B, d))), T(det(pfx + "kv", (S, B, d)))
    w = T(det(pfx + "w", (Tn, B, d)))
    x, kv = x0.clone().requires_grad_(True), kv0.clone().requires_grad_(True)
    y_ref = O.encoder(sd, "", O.EncCfg(H, Ly, attn_mask=mask, biprojection=bi), x, kv, kv)
    (y_ref * w).sum().backward()
    enc = enc.cuda().train()
    xg, kvg = x0.cuda().requires_grad_(True), kv0.cuda().requires_grad_(True)
    y = enc(xg, kvg, kvg)
    (y * w.cuda()).sum().backward()
    pairs = [("y", y, y_ref), ("gx", xg.grad, x.grad), ("gkv", kvg.grad, kv.grad)] + \
            [(k, p.grad, sd[k].grad) for k, p in enc.named_parameters()]
    worst = ("", 0.0)
    for what, a, b in pairs:
        assert a is not None and b is not None, what
        if prec == "f32":
            err = float((a.detach().cpu().double() - b.detach().double()).abs().max())
            assert err <= 2e-4 * max(1.0, float(b.detach().abs().max())), f"{what}: max err {err:.3e}"
        else:
            r = _rel(a, b)
            worst = max(worst, (what, r), key=lambda t: t[1])
            lim = 1e-2 if what == "y" else 1e-1 if what in ("gx", "gkv") else 2e-1 if "layer_norm" in what else 1.4e-1
            assert r <= lim, f"{what}: rel-L2 {r:.3e} > {lim}"
    if prec == "bf16":
        _record(f"wide_encoder/{pfx}", prec, {"worst": worst[0], "rel_l2": worst[1]})


@pytest.mark.parametrize("prec,B", [("f32", 3), ("bf16", 2), ("bf16x3", 2)])
def test_low_rank_key_side_equals_the_dk_dv_route_at_head_dim_256(prec, B):
    """test_model_gpu.py's low-rank / dK-dV comparison at hidden 512, 2 heads (head_dim 256): level 2 of the pruned 3-modal
    model in training mode with every dropout on, same weights, inputs and seeds on both routes."""
    from bpmult_amd import engine
    torch.manual_seed(5)
    a = args_for("mmtrvat", hidden_sz=512, num_heads=2, layers=2, orig_d_l=32, num_vectors_l=96, num_vectors_a=96,
                 num_vectors_v=96, attn_dropout=0.2, attn_dropout_a=0.1, attn_dropout_v=0.15)
    xs = [torch.randn(B, 40, 32), torch.randn(B, 96, 35), torch.randn(B, 77, 74)]
    m1 = get_model(a)
    with torch.no_grad():
        for p in m1.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    m2 = copy.deepcopy(m1)
    tgt = (torch.randn(B, a.n_classes) > 0).float().cuda()
    outs = []
    keep = engine._LOWRANK
    try:
        for m, lowrank in ((m1, False), (m2, True)):
            engine._LOWRANK = lowrank
            m.precision = prec
            m = m.cuda().train()
            m.set_prune_unused_rows(True)
            x = [t.clone().cuda().requires_grad_(True) for t in xs]
            logits, z = m(x[0], None, None, *x[1:], output_gate=True)
            assert m._trunks[B].plan2._lowrank == lowrank and m._trunks[B].plan2.dhp == 256
            torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt).backward()
            outs.append((logits.detach(), z.detach(), {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None},
                         [t.grad.detach().clone() for t in x]))
    finally:
        engine._LOWRANK = keep
    assert torch.equal(outs[0][0], outs[1][0]) and torch.equal(outs[0][1], outs[1][1]), "forward is the same launch sequence"
    tol_g = {"f32": 5e-6, "bf16x3": 5e-6, "bf16": 1.5e-2}[prec]      # the limits of the head_dim <= 128 test
    worst = ("", 0.0)
    for k in outs[0][2]:
        g0, g1 = outs[0][2][k], outs[1][2][k]
        if float(g0.norm()) < 1e-9:
            assert float(g1.norm()) < 1e-6, k
            continue
        r = _rel(g1, g0)
        worst = max(worst, (k, r), key=lambda t: t[1])
        assert r <= tol_g, (k, r)
    for g0, g1 in zip(outs[0][3], outs[1][3]):
        assert _rel(g1, g0) <= tol_g
    _record("lowrank_vs_dkdv_dh256/", prec, {"worst_gradient": worst[0], "rel_l2": worst[1]})


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_graph_replay_equals_eager_launches_at_head_dim_256(prec):
    """The captured step (forward + backward graphs, dropout seed read at execution time) gives bit-for-bit the logits,
    gates and gradients of eager launches at hidden 512 / 2 heads, README dropout rates on, over several micro-steps."""
    torch.manual_seed(3)
    a = args_for("mmtrvat", hidden_sz=512, num_heads=2, layers=2, orig_d_l=32, num_vectors_l=48, num_vectors_a=48,
                 num_vectors_v=48, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.25, out_dropout=0.1)
    m1 = get_model(a)
    m1.precision = prec
    m2 = copy.deepcopy(m1)
    m1, m2 = m1.cuda().train(), m2.cuda().train()
    m1.use_graphs, m2.use_graphs = False, True
    gen = torch.Generator().manual_seed(4)
    x = [torch.randn(2, 17, 32, generator=gen).cuda(), torch.randn(2, 48, 35, generator=gen).cuda(),
         torch.randn(2, 31, 74, generator=gen).cuda()]
    tgt = (torch.randn(2, 6, generator=gen) > 0).float().cuda()
    for step in range(5):
        outs = []
        for m in (m1, m2):
            for p in m.parameters():
                p.grad = None
            xs = [t.clone().requires_grad_(True) for t in x]
            logits, z = m(xs[0], None, None, xs[1], xs[2], output_gate=True)
            torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt).backward()
            outs.append((logits.detach().clone(), z.detach().clone(), [t.grad.clone() for t in xs],
                         {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
        a_, b_ = outs
        assert torch.equal(a_[0], b_[0]) and torch.equal(a_[1], b_[1]), f"step {step}: logits / gates differ"
        for u, v in zip(a_[2], b_[2]):
            assert torch.equal(u, v), f"step {step}: input gradients differ"
        for k in a_[3]:
            if "gmu." in k or k.startswith(("proj1", "proj2", "out_layer")) or "layer_norm" in k or "bias" in k:
                # float atomics / two-stream arrival order in the tail and the column sums (as test_model_gpu.py)
                assert float((a_[3][k] - b_[3][k]).abs().max()) <= 1e-5 * max(1.0, float(a_[3][k].abs().max())), (step, k)
            else:
                assert torch.equal(a_[3][k], b_[3][k]), f"step {step}: gradient of {k} differs"
    assert any("graph" in e for e in m2._trunks[2]._fg.values()), "the step was captured"
