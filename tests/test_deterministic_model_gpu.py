"""Deterministic mode on the MI355X: same seed, same bits -- every parameter gradient with no exception list, three
FusedAdam steps, eager launches against graph replay; for the 3-modal and the 4-modal model of
tests/test_plan_tables_cpu.py (hidden 64 and 40, 2 layers, B = 2, dropout on) in f32 and bf16 and both schedules, the
stand-alone MultiheadAttention (cases k2 and, for the projection biases k2 lacks, k1 of tests/mha_kpm_cases.py) and the
HIP BertEncoder with HIP embeddings (both with three torch.optim.Adam steps: FusedAdam and graph replay are the trunk's).
Deterministic against default mode (f32, same seed): logits and every tensor no route touches bit-equal, the re-routed
sums within rtol 1e-5 of the tensor's scale, the figure the project's tests hold these sums to."""
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

import bpmult_amd  # noqa: E402,F401
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.models.bpmult import LEVEL2  # noqa: E402

DEV = "cuda"


def _args(model, **kw):
    a = dict(model=model, orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=64, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0.1, attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.1, res_dropout=0.1,
             out_dropout=0., embed_dropout=0.25, attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
             text_features=True, precision="bf16", num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


CASES = {"three": ("mmtrvat", {}), "four": ("mmtrvapt", {"orig_d_a": 96, "hidden_sz": 40, "num_vectors_a": 40, "num_vectors_v": 40})}


def build(case, prec, prune, deterministic=True, graphs=False, seed=11):
    """A model and its inputs, both from `seed` (the dropout seeds follow torch's initial seed and the model's step count)."""
    name, kw = CASES[case]
    torch.manual_seed(seed)
    m = get_model(_args(name, prune_unused_rows=prune, precision=prec, deterministic=deterministic, **kw))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():                                # biases and LayerNorm affines away from their 0 / 1 initial values
        for k, p in m.named_parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn(p.shape, generator=g))
    if case == "four":
        m.audio_enc.conv_layers[2] = torch.nn.AdaptiveAvgPool1d(40)
        x = [torch.randn(2, 17, 32, generator=g), torch.randn(2, 30, 35, generator=g), torch.randn(2, 96, 600, generator=g),
             torch.randn(2, 64, generator=g)]
    else:
        x = [torch.randn(2, 17, 32, generator=g), torch.randn(2, 48, 35, generator=g), torch.randn(2, 31, 74, generator=g)]
    m = m.cuda().train()
    m.use_graphs = graphs
    return m, [t.cuda() for t in x]


def fwd_bwd(m, x):
    out = m(x[0], None, None, *x[1:])
    out.square().mean().backward()
    return out.detach()


def grads(m):
    torch.cuda.synchronize()
    return {n: p.grad.detach().clone() for n, p in m.named_parameters() if p.grad is not None}


def assert_same(a, b, what):
    assert set(a) == set(b), what
    bad = [n for n in a if not torch.equal(a[n], b[n])]
    assert not bad, f"{what}: {len(bad)} of {len(a)} tensors differ, first {bad[:6]}"


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "dense"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_two_models_from_one_seed_agree_bit_for_bit(case, prec, prune):
    from bpmult_amd.optim import FusedAdam
    runs = []
    for _ in range(2):
        m, x = build(case, prec, prune)
        assert m._trunk_for(2).plan1.det and m._trunk_for(2).plan2.det
        out = fwd_bwd(m, x)
        g1 = grads(m)
        assert len(g1) > 100 and all(torch.isfinite(t).all() for t in g1.values())
        opt = FusedAdam(m, lr=1e-2)
        outs = []
        for _ in range(3):
            opt.zero_grad()
            outs.append(fwd_bwd(m, x))
            opt.step()
        torch.cuda.synchronize()
        runs.append((out, g1, outs, {n: p.detach().clone() for n, p in m.named_parameters()}))
    a, b = runs
    assert torch.equal(a[0], b[0]), "logits"
    assert_same(a[1], b[1], "parameter gradients of one forward + backward")
    assert all(torch.equal(p, q) for p, q in zip(a[2], b[2])), "logits of the three steps"
    assert_same(a[3], b[3], "parameters after three FusedAdam steps")


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "dense"])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_graph_replay_equals_eager_launches(case, prec, prune):
    """Four steps each (GraphCache.GRAPH_WARMUP = 2: the third call captures, the fourth replays)."""
    from bpmult_amd.graphs import GraphCache
    from bpmult_amd.optim import FusedAdam
    assert GraphCache.GRAPH_WARMUP == 2
    runs = []
    for graphs in (False, True):
        m, x = build(case, prec, prune, graphs=graphs)
        opt = FusedAdam(m, lr=1e-2)
        outs, gs = [], []
        for _ in range(4):
            opt.zero_grad()
            outs.append(fwd_bwd(m, x))
            gs.append(grads(m))
            opt.step()
        torch.cuda.synchronize()
        runs.append((outs, gs, {n: p.detach().clone() for n, p in m.named_parameters()}))
    (oa, ga, pa), (ob, gb, pb) = runs
    for k in range(4):
        assert torch.equal(oa[k], ob[k]), f"logits of step {k}"
        assert_same(ga[k], gb[k], f"gradients of step {k}")
    assert_same(pa, pb, "parameters after four steps")


def _rerouted(name, four):
    """The gradients whose sum takes another route in deterministic mode."""
    if name.endswith((".fc1.bias", ".fc2.bias", ".self_attn.out_proj.bias")):
        return True
    parts = name.split(".")
    if len(parts) == 6 and parts[1] == "layers" and parts[3] == "layer_norms":      # the key / value LayerNorm: unfold_grads
        return int(parts[4]) == (1 if four and parts[0] in LEVEL2 else 0)
    return False


@pytest.mark.parametrize("prune", [True, False], ids=["pruned", "dense"])
@pytest.mark.parametrize("case", sorted(CASES))
def test_deterministic_against_default_mode_f32(case, prune):
    md, x = build(case, "f32", prune, deterministic=True)
    od = fwd_bwd(md, x)
    gd = grads(md)
    m0, x0 = build(case, "f32", prune, deterministic=False)
    assert not m0._trunk_for(2).plan1.det
    o0 = fwd_bwd(m0, x0)
    g0 = grads(m0)
    assert torch.equal(od, o0), "logits"
    assert set(gd) == set(g0)
    n_routed, bad = 0, []
    for n in gd:
        if _rerouted(n, case == "four"):
            n_routed += 1
            scale = float(g0[n].abs().max())
            err = float((gd[n] - g0[n]).abs().max())
            print(f"{n}: |det - default| {err:.3e} at scale {scale:.3e}")
            if err > 1e-5 * scale:
                bad.append(f"{n}: {err:.3e} > 1e-5 x {scale:.3e}")
        elif not torch.equal(gd[n], g0[n]):
            bad.append(f"{n}: not bit-equal")
    assert n_routed == 12 * 2 * 5, n_routed          # twelve encoders x two layers x (three biases + the LayerNorm's affine pair)
    assert not bad, "\n  ".join(bad)


def _mha_run(tag, prec, deterministic):
    """One forward + backward, then three Adam steps, of a fresh module under one dropout seed -> every tensor of the first
    step, the gradients of each later step, the parameters at the end."""
    from mha_kpm_cases import case
    from test_mha_kpm_module_gpu import build as build_mha, step
    m, a = build_mha(case(tag), prec, dropout=0.1, train=True)
    m.deterministic = deterministic
    torch.manual_seed(5)
    m._step = 0
    first = step(m, a)
    assert m._exec.det is deterministic
    opt = torch.optim.Adam(m.parameters(), lr=1e-2)
    later = []
    for _ in range(3):
        out = step(m, a)                                  # (clears the gradients first)
        later.append({n: t for n, t in out.items() if n.startswith("g.") and t is not None})
        opt.step()
    torch.cuda.synchronize()
    return first, later, {n: p.detach().clone() for n, p in m.named_parameters()}


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", ["k2", "k1"])
def test_multihead_attention(tag, prec):
    """Two modules from the same weights under one dropout seed: every tensor of a forward + backward, the gradients of
    three optimizer steps and the parameters after them, bit for bit.  k2 (d = 50) has no projection biases, k1 has
    them: their gradients are compared like everything else.  (The stand-alone module has no flat store and no graph
    cache -- FusedAdam and graph replay belong to the models' trunk -- so the steps are torch.optim.Adam's, eager.)"""
    (x, xl, xp), (z, zl, zp) = _mha_run(tag, prec, True), _mha_run(tag, prec, True)
    assert ("g.out_proj.bias" in x and "g.in_proj_bias" in x) == (tag == "k1")
    bad = [n for n in x if x[n] is not None and not torch.equal(x[n], z[n])]
    bad += [f"step {k}: {n}" for k, (a, b) in enumerate(zip(xl, zl)) for n in a if not torch.equal(a[n], b[n])]
    bad += [f"parameter {n}" for n in xp if not torch.equal(xp[n], zp[n])]
    assert not bad, (prec, bad)
    if prec != "f32":
        return
    y = _mha_run(tag, prec, False)[0]                     # default mode, same seed, f32: only d(out_proj.bias) takes another route
    for n in x:
        if x[n] is None:
            continue
        if n == "g.out_proj.bias":
            assert float((x[n] - y[n]).abs().max()) <= 1e-5 * float(y[n].abs().max()), (prec, n)
        else:
            assert torch.equal(x[n], y[n]), (prec, n)     # g.in_proj_bias too: colsum_a of the in_proj products in both modes


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_hip_bert_encoder(tmp_path, prec):
    import test_text_encoder_gpu as T
    from test_text_embeddings_gpu import _enc_step
    from bpmult_amd.models.bpmult import BertEncoder
    T.build("small", dropout=0.1).save_pretrained(tmp_path / "bert")
    ids, mask, seg, w = (t.to(DEV) for t in T.inputs("small"))
    runs = []
    for _ in range(2):
        enc = BertEncoder(SimpleNamespace(bert_model=str(tmp_path / "bert"), text_features=False, text_encoder="hip",
                                          text_embeddings="hip", precision=prec, deterministic=True)).to(DEV).train()
        assert enc.deterministic is True
        first = _enc_step(enc, ids, mask, seg, w)
        assert all(pl.det for pl in enc._stack._plans.values())
        opt = torch.optim.Adam([p for n, p in enc.bert.named_parameters() if not n.startswith("pooler.")], lr=1e-3)
        later = []
        for _ in range(3):                            # three optimizer steps (torch's Adam: the module alone has no flat store)
            later.append(_enc_step(enc, ids, mask, seg, w))
            opt.step()
        torch.cuda.synchronize()
        runs.append((first, later, {n: p.detach().clone() for n, p in enc.bert.named_parameters()}))
    ((oa, ga), la, pa), ((ob, gb), lb, pb) = runs
    assert torch.equal(oa, ob)
    assert set(ga) == set(gb) and all(v is not None for v in ga.values())
    bad = [n for n in ga if not torch.equal(ga[n], gb[n])]
    for k, ((o1, g1), (o2, g2)) in enumerate(zip(la, lb)):
        bad += [f"step {k}: out"] * (not torch.equal(o1, o2)) + [f"step {k}: {n}" for n in g1 if not torch.equal(g1[n], g2[n])]
    bad += [f"parameter {n}" for n in pa if not torch.equal(pa[n], pb[n])]
    assert not bad, bad
