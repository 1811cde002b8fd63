"""Training across optimizer steps, graph replay and bf16x3 split images: every step of a scripted run against the CPU
oracle (oracle.bpmult_cpu.bpmult3_forward, fp32 autograd) evaluated at the model's CURRENT state_dict() on the same batch.

The single-step parity tests (tests/test_model_gpu.py) load weights and run one forward + backward.  What exists only to
avoid recomputation across steps sits between steps: the weight shadows the optimizer kernel writes and the next forward's
rest refresh completes, the buffers captured graphs point into, and the bf16x3 split images (ops._X3Plan).  A stale one gives
finite, plausible numbers.  Here the weights are re-synchronised into the oracle before every step, so Adam's amplification
of rounding noise never enters: a mismatch at step k is a stale shadow / image / graph buffer of step k.

The script (fresh random inputs every step, targets that alternate between a class pattern and its complement -- see LR --,
optimizer step after each; GraphCache.GRAPH_WARMUP = 2, so shape A is
captured on its third call): steps 0-2 shape A; 3 shape A, a pure replay; 4 shape B (another video length); 5 shape A, two
accumulating micro-steps; 6 after an in-place edit of one weight matrix and one LayerNorm gain (the version-counter path:
full refresh); 7 after an eval() forward under no_grad (compared too), back in train().

Limits: the ones tests/test_model_gpu.py holds each precision to for ONE step (its `check`): f32 1e-4 abs on logits / gates /
loss and 2e-3 of the tensor's max on gradients; bf16x3 X3_FWD / X3_GRAD of the tensor's max; bf16 relative L2 BF16_FWD and
BF16_GRAD_TOY.  Each check must be able to see a stale step: from step 1 on the oracle is also evaluated at the PREVIOUS
step's weights on the current batch, and that stale reference must differ from the current one by >= 10x the limit (f32 /
bf16x3: logits and every gradient tensor that is not negligible; bf16: logits and loss only -- its per-tensor gradient
limits, 0.4 relative L2, are too loose for a 10x margin).  That is a condition on the reference alone.

Measured errors and stale ratios: profiles/r10_training_steps.json (a copy of what this file writes beside
test_model_gpu.PARITY_LOG)."""
import json
import os
import re

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_model_gpu import BF16_FWD, BF16_GRAD_TOY, PARITY_LOG, X3_FWD, X3_GRAD, args_for  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import ops  # noqa: E402
from bpmult_amd._lib import GEMM_NN, GEMM_NT, GEMM_TN  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from oracle import bpmult_cpu as O  # noqa: E402

LOG = os.path.join(os.path.dirname(PARITY_LOG), "r10_training_steps.json")

BCE = torch.nn.functional.binary_cross_entropy_with_logits
# The data and the optimizer settings are chosen so that the ORACLE satisfies the stale condition at every step (rehearsed on
# the CPU with the oracle alone).  With random targets the loss of a fresh batch moves by a random, often tiny amount per
# step, and bf16 needs a loss that moves by >= 25 %: so the targets alternate -- step k asks for a fixed class pattern when
# k is even and for its complement when k is odd -- and beta1 = 0, so that every step moves all logits towards the pattern
# the NEXT step contradicts (with momentum 0.9 the alternating gradients cancel and the steps shrink twentyfold).  The
# weights one step back are then better (or worse) on the current batch by a margin that does not depend on the draw.
# Measured on the oracle's own trajectory (its gradients fed to torch.optim.Adam): smallest stale ratio 12.2 (f32 toy, a
# LayerNorm gain at step 7; >= 27 before), 26 (bf16 toy, the loss at step 1), 14.6 (bf16x3 at hidden 512, lr 7e-4: larger
# rates saturate the gates and shrink the gradients).
LR = {"f32": 3e-2, "bf16x3": 7e-4, "bf16": 3e-2}
BETAS = (0.0, 0.999)
STALE_FACTOR = 10.0
# fc1 biases +-4 (alternating units).  The pre-activations W x of a normalised row are ~N(0, 1) here, so a unit is on or
# off by a wide margin.  Without this the reference itself is not defined to the limits: a ReLU unit whose pre-activation
# is within rounding of zero has a gate that rounding decides, the gradient reaches the encoders through two time steps
# only (the fusion reads rows 0 and N-1), and ONE such unit in one of those rows moves fc1.weight's gradient by ~1 % of
# its largest entry.  Measured on the oracle alone at hidden 512: weights perturbed by 3e-6 relative move
# trans_a_with_v.layers.0.fc1.weight's gradient by 2.4x the bf16x3 limit and fc1.bias's by 2.0x -- to the digit what the
# HIP path showed at step 0, before any optimizer step, with biases 0 (about one such unit every other step at that size).
RELU_OFFSET = 4.0
# a gradient tensor is "negligible" for the stale condition when its largest reference entry is below this fraction of
# the largest entry of any gradient tensor of the step (sums of cancelling terms: nothing to tell a stale step by)
NEGLIGIBLE = 1e-4

# toy: tests/test_model_gpu.py's small mmtrvat (lengths that are no whole 64-key tile).  x3: the smallest mmtrvat whose
# level-1 launches take the split path in all three operand arrangements -- ops._X3Plan._eligible needs M, N, K >= 256
# (rows = vectors * B = 256, hidden 512) and a TN launch 96 tiles of 256 x 256 (six encoders x (fc1 + fc2: 8 tiles each)
# = 96; at hidden 256 or 384 no weight-gradient launch reaches that)
SHAPES = {
    "toy": dict(hidden=48, heads=4, layers=2, nvec=96, L=40, V=96, VB=80, A=77),
    "x3": dict(hidden=512, heads=8, layers=1, nvec=128, L=40, V=128, VB=100, A=97),
}
ORIG_L, ORIG_V, ORIG_A, NCLS, B = 32, 35, 74, 6, 2


# ---- model, data, reference (CPU only: importable without a GPU) ---------------------------------------------------
def build_model(shape, prec, seed=17):
    """Weights: the model's own initialisation, then fc1 / fc2 / in_proj weights drawn N(0, 1 / fan_in) and LayerNorm gains
    1 + 0.1 N, so that every tensor's gradient moves by a large fraction from one optimizer step to the next."""
    s = SHAPES[shape]
    torch.manual_seed(seed)
    m = get_model(args_for("mmtrvat", hidden_sz=s["hidden"], num_heads=s["heads"], layers=s["layers"], orig_d_l=ORIG_L,
                           num_vectors_l=s["nvec"], num_vectors_a=s["nvec"], num_vectors_v=s["nvec"], n_classes=NCLS))
    g = torch.Generator().manual_seed(seed + 1)
    with torch.no_grad():
        for k, p in m.named_parameters():
            if re.search(r"layers\.\d+\.(fc1\.weight|fc2\.weight|self_attn\.in_proj_weight)$", k):
                p.copy_(torch.randn(p.shape, generator=g) * p.shape[1] ** -0.5)
            elif re.search(r"layer_norms?(\.\d+)?\.weight$", k):
                p.copy_(1 + 0.1 * torch.randn(p.shape, generator=g))
            elif re.search(r"layers\.\d+\.fc1\.bias$", k):
                p.copy_(RELU_OFFSET * (1 - 2 * (torch.arange(p.numel()) % 2)).float())
    m.precision = prec
    return m


def oracle_cfg(shape):
    s = SHAPES[shape]
    return O.ModelCfg(s["hidden"], s["heads"], s["layers"], NCLS, orig_d_l=ORIG_L, orig_d_v=ORIG_V, orig_d_a=ORIG_A,
                      num_vectors_l=s["nvec"], num_vectors_a=s["nvec"], num_vectors_v=s["nvec"])


def batch(shape, step, micro=0, other_video=False):
    """Fresh random inputs; targets: the class pattern 0 1 0 1 .. at even steps, its complement at odd ones (see LR)."""
    s = SHAPES[shape]
    g = torch.Generator().manual_seed(1000 * step + 10 * micro + 7)
    V = s["VB"] if other_video else s["V"]
    tgt = ((torch.arange(NCLS) + step) % 2).float().expand(B, NCLS).contiguous()
    return dict(xl=torch.randn(B, s["L"], ORIG_L, generator=g), img=torch.randn(B, V, ORIG_V, generator=g),
                aud=torch.randn(B, s["A"], ORIG_A, generator=g), tgt=tgt)


# (step, micro-batches, event before the step)
def script(shape, steps=8):
    plan = [(0, 1, None), (1, 1, None), (2, 1, None), (3, 1, None), (4, 1, "shape_b"), (5, 2, None), (6, 1, "edit"), (7, 1, "eval")]
    return [(k, [batch(shape, k, j, other_video=(ev == "shape_b")) for j in range(n)], ev) for k, n, ev in plan[:steps]]


def snapshot(model):
    return {k: v.detach().cpu().clone() for k, v in model.state_dict().items() if v.dtype == torch.float32}


def reference(sd, cfg, micro, training=True, grads=True):
    """The oracle at weights `sd` on the micro-batches of one step: per micro-batch logits / gates / loss / input gradients,
    and the parameter gradients summed over the micro-batches (what accumulation leaves in .grad)."""
    w = {k: v.clone().requires_grad_(grads) for k, v in sd.items()}
    out = dict(logits=[], z=[], loss=[], gin=[])
    xs, total = [], 0
    with torch.set_grad_enabled(grads):
        for b in micro:
            x = {k: b[k].clone().requires_grad_(grads) for k in ("xl", "img", "aud")}
            logits, z = O.bpmult3_forward(w, cfg, x["xl"], x["img"], x["aud"], training=training)
            loss = BCE(logits, b["tgt"])
            total = total + loss
            xs.append(x)
            out["logits"].append(logits.detach().numpy())
            out["z"].append(z.detach().numpy())
            out["loss"].append(loss.detach().numpy())
        if grads:
            total.backward()
    if grads:
        out["gin"] = [{k: t.grad.numpy() for k, t in x.items()} for x in xs]
        out["g"] = {k: (t.grad.numpy() if t.grad is not None else None) for k, t in w.items()}
    return out


def measure(a, b, prec, kind):
    """(error, limit) of `a` against the reference `b` as tests/test_model_gpu.py's `check` takes them for this precision:
    kind "fwd" (logits, gates, loss) or "grad"."""
    a, b = np.asarray(a, dtype=np.float32), np.asarray(b, dtype=np.float32)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all()
    scale = max(float(np.abs(b).max()), 1e-6)
    if prec == "bf16":
        rel = float(np.linalg.norm((a - b).ravel()) / max(np.linalg.norm(b.ravel()), 1e-12))
        return rel, (BF16_FWD if kind == "fwd" else BF16_GRAD_TOY)
    e = float(np.abs(a - b).max())
    if prec == "bf16x3":
        return e, (X3_FWD if kind == "fwd" else X3_GRAD) * max(scale, 1e-3)
    return e, (1e-4 if kind == "fwd" else 2e-3 * max(scale, 1e-3))


def stale_ratios(cur, stale, prec):
    """{quantity: (current reference - stale reference) / limit}: how far a step computed with the previous weights would be
    from the reference, in units of what the parity check allows.  bf16: logits and loss only."""
    r = {}
    for j, (c, s) in enumerate(zip(cur["logits"], stale["logits"])):
        d, lim = measure(s, c, prec, "fwd")
        r[f"logits.{j}"] = d / lim
    if prec == "bf16":
        for j, (c, s) in enumerate(zip(cur["loss"], stale["loss"])):
            d, lim = measure(s, c, prec, "fwd")
            r[f"loss.{j}"] = d / lim
        return r
    tensors = {"g." + k: (cur["g"][k], stale["g"][k]) for k in cur["g"] if cur["g"][k] is not None}
    for j, (c, s) in enumerate(zip(cur["gin"], stale["gin"])):
        tensors.update({f"gin.{k}.{j}": (c[k], s[k]) for k in c})
    top = max(float(np.abs(c).max()) for c, _ in tensors.values())
    for k, (c, s) in tensors.items():
        if float(np.abs(c).max()) < NEGLIGIBLE * top:
            continue
        d, lim = measure(s, c, prec, "grad")
        r[k] = d / lim
    return r


def edit_weights(model):
    """Step 6's in-place edit (version counters, not the optimizer: the full shadow refresh)."""
    with torch.no_grad():
        model.trans_l_with_a.layers[0].fc1.weight.mul_(-1.5)
        model.trans_v_with_a.layers[0].layer_norms[0].weight.mul_(0.5)


# ---- the GPU run ---------------------------------------------------------------------------------------------------
_RESULTS = {}


def _write_log(key, rec):
    _RESULTS[key] = rec
    try:
        os.makedirs(os.path.dirname(LOG), exist_ok=True)
        old = {}
        if os.path.exists(LOG):
            with open(LOG) as f:
                old = json.load(f)
        old.update(_RESULTS)
        with open(LOG, "w") as f:
            json.dump(old, f, indent=1, sort_keys=True)
    except OSError:
        pass


def run_script(shape, prec, graphs, fused, prune, monkeypatch, steps=8):
    from bpmult_amd.graphs import GraphCache
    from bpmult_amd.optim import FusedAdam
    assert GraphCache.GRAPH_WARMUP == 2, "the script expects shape A to be captured on its third call"
    cfg = oracle_cfg(shape)
    model = build_model(shape, prec)
    model.set_prune_unused_rows(prune)
    model = model.cuda().train()
    model.use_graphs = graphs
    opt = FusedAdam(model, lr=LR[prec], betas=BETAS) if fused else torch.optim.Adam(model.parameters(), lr=LR[prec], betas=BETAS)

    now = {"step": -1}
    x3_runs, replays = {}, {}
    plan_run, graph_replay = ops._X3Plan.run, torch.cuda.CUDAGraph.replay

    def counted_run(self, L, variant, seed, s):
        assert self.ok
        x3_runs.setdefault(now["step"], set()).add(variant)
        return plan_run(self, L, variant, seed, s)

    def counted_replay(self):
        replays[now["step"]] = replays.get(now["step"], 0) + 1
        return graph_replay(self)

    monkeypatch.setattr(ops._X3Plan, "run", counted_run)
    monkeypatch.setattr(torch.cuda.CUDAGraph, "replay", counted_replay)

    rec = {"errors": {}, "stale_ratio_min": {}}
    failures = []
    prev = None
    shape_a_key = None

    def compare(step, what, got, ref, kind):
        e, lim = measure(got.detach().float().cpu().numpy(), ref, prec, kind)
        q = what.split(".")[0] if kind == "fwd" else ("gin" if what.startswith("gin.") else "grad")
        w = rec["errors"].setdefault(q, {}).setdefault(str(step), {"error": 0.0, "limit": lim, "ratio": -1.0, "what": ""})
        if e / lim > w["ratio"]:
            w.update(error=e, limit=lim, ratio=e / lim, what=what)
        if not e <= lim:
            failures.append(f"step {step}: {what}: error {e:.3e} > limit {lim:.3e}")

    for step, micro, event in script(shape, steps):
        now["step"] = step
        if event == "edit":
            after_opt = snapshot(model)
            edit_weights(model)
        if event == "eval":
            model.eval()
            b = batch(shape, 100 + step)
            with torch.no_grad():
                out = model(b["xl"].cuda(), None, None, b["img"].cuda(), b["aud"].cuda())
            ref = reference(snapshot(model), cfg, [b], training=False, grads=False)
            compare(step, "logits.eval", out, ref["logits"][0], "fwd")
            model.train()
        sd = snapshot(model)
        cur = reference(sd, cfg, micro)
        # -- the condition on the reference alone: a step computed at stale weights would be seen
        if prev is not None:
            ratios = stale_ratios(cur, reference(prev, cfg, micro), prec)
            if event == "edit":           # ... and so would a step that missed only the in-place edit (f32 / bf16x3)
                miss = reference(after_opt, cfg, micro, grads=False)
                if prec != "bf16":
                    d, lim = measure(miss["logits"][0], cur["logits"][0], prec, "fwd")
                    ratios["logits.0.without_the_edit"] = d / lim
            k = min(ratios, key=ratios.get)
            rec["stale_ratio_min"][str(step)] = {"ratio": ratios[k], "what": k, "tensors": len(ratios)}
            assert ratios[k] >= STALE_FACTOR, f"step {step}: the stale reference is within {ratios[k]:.2f}x the limit at {k}"
        assert all(float(l) > 1e-2 for l in cur["loss"]), cur["loss"]
        prev = sd
        # -- the step on the GPU
        was_captured = graphs and shape_a_key is not None and "graph" in model._trunks[B]._fg.get(shape_a_key, {})
        opt.zero_grad()
        xs_all = []
        for j, b in enumerate(micro):
            xs = {k: b[k].cuda().requires_grad_(True) for k in ("xl", "img", "aud")}
            logits, z = model(xs["xl"], None, None, xs["img"], xs["aud"], output_gate=True)
            loss = BCE(logits, b["tgt"].cuda())
            loss.backward()
            xs_all.append(xs)
            compare(step, f"logits.{j}", logits, cur["logits"][j], "fwd")
            compare(step, f"z.{j}", z, cur["z"][j], "fwd")
            compare(step, f"loss.{j}", loss, cur["loss"][j], "fwd")
        for j, xs in enumerate(xs_all):
            for k, t in xs.items():
                compare(step, f"gin.{k}.{j}", t.grad, cur["gin"][j][k], "grad")
        for k, p in model.named_parameters():
            if cur["g"][k] is None:
                assert p.grad is None or float(p.grad.abs().max()) == 0.0, k
            else:
                assert p.grad is not None, k
                compare(step, "g." + k, p.grad, cur["g"][k], "grad")
        opt.step()
        trunk = model._trunks[B]
        if step == 0:
            s = SHAPES[shape]
            shape_a_key = (True, ((B, s["L"], ORIG_L), (B, s["V"], ORIG_V), (B, s["A"], ORIG_A)), False)
        if graphs:
            assert shape_a_key in trunk._fg
            if step == 3:                          # a pure replay: forward graph (captured at step 2) and backward graph
                assert was_captured and replays.get(step, 0) == 2, (was_captured, replays)
        if prec == "bf16x3" and not (graphs and was_captured and event != "shape_b"):
            # (a replay runs no Python: its launches are those of the capture, counted at step 2)
            assert x3_runs.get(step) == {GEMM_NT, GEMM_NN, GEMM_TN}, f"step {step}: split launches ran for {x3_runs.get(step)}"

    tag = f"{prec}/{shape}.graphs{int(graphs)}.{'fused' if fused else 'torch'}adam.{'pruned' if prune else 'dense'}"
    if graphs:
        ent = trunk._fg[shape_a_key]
        st = trunk.graph_stats
        n_a = sum(len(m_) for _, m_, ev in script(shape, steps) if ev != "shape_b")
        assert "graph" in ent and st["failed"] == 0 and st["captured"] >= 1, (st, list(ent))
        assert ent["calls"] == n_a and sum(replays.values()) >= n_a - GraphCache.GRAPH_WARMUP, (ent["calls"], replays)
        assert any(bk[0] == shape_a_key and "graph" in e for bk, e in trunk._bg.items()), "shape A's backward was captured"
        rec["graph"] = {"captured": st["captured"], "shape_a_calls": ent["calls"], "replays_per_step": {str(k): v for k, v in replays.items()}}
    else:
        assert not replays and not getattr(trunk, "_fg", None)
    if prec == "bf16x3":
        assert len(x3_runs) >= 2 and max(x3_runs) >= 1, "split launches after the first optimizer step"
        rec["x3_steps_with_split_launches"] = sorted(x3_runs)
    _write_log(tag, rec)
    assert not failures, "\n".join(failures)


GRAPHS_OFF = os.environ.get("BPMULT_GRAPH", "1") == "0"
_graph = lambda on: pytest.param(on, id=f"graphs{int(on)}", marks=pytest.mark.skipif(
    on and GRAPHS_OFF, reason="graph replay switched off by BPMULT_GRAPH=0"))


@pytest.mark.parametrize("fused", [pytest.param(True, id="fusedadam"), pytest.param(False, id="torchadam")])
@pytest.mark.parametrize("graphs", [_graph(True), _graph(False)])
@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_training_steps_match_the_oracle(prec, graphs, fused, monkeypatch):
    """Toy mmtrvat (hidden 48, 4 heads, 2 layers, 96 vectors, B = 2), default (pruned) schedule, the eight scripted steps."""
    run_script("toy", prec, graphs, fused, True, monkeypatch)


@pytest.mark.parametrize("graphs,fused,prune", [
    pytest.param(True, True, True, id="graphs1-fusedadam-pruned", marks=pytest.mark.skipif(GRAPHS_OFF, reason="graph replay switched off by BPMULT_GRAPH=0")),
    pytest.param(False, True, False, id="graphs0-fusedadam-dense"),
    pytest.param(True, False, True, id="graphs1-torchadam-pruned", marks=pytest.mark.skipif(GRAPHS_OFF, reason="graph replay switched off by BPMULT_GRAPH=0")),
])
def test_training_steps_bf16x3_split_path(graphs, fused, prune, monkeypatch):
    """bf16x3 at the smallest mmtrvat whose launches really take the split path (hidden 512, 8 heads, 1 layer, 128 vectors,
    B = 2: SHAPES["x3"]); every eager step asserts split launches of all three operand arrangements."""
    run_script("x3", "bf16x3", graphs, fused, prune, monkeypatch)
