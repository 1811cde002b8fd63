"""The BERT layer stack on the HIP path (`args.text_encoder = "hip"`, models/bert.py) on the MI355X against HF
`BertModel` itself in fp64 on the CPU: last hidden state at ALL positions (padded ones included), the gradient of every
layer parameter and of the embedding output, under a loss that weights every position.

Error measure of one tensor: max |got - ref| / max(max |ref|, floor); the floor only matters for parameter gradients
that are zero in exact arithmetic (a key bias shifts every score of a row alike): 1e-3 of the largest parameter gradient.
Reported: "out" (hidden state), "demb" (embedding-output gradient), "per" (EVERY layer parameter's gradient, by name;
"dparam" / "worst_param" name the worst one for reading).  Every tensor is held to ITS OWN recorded figure: a weight
gradient is not excused by the noise of a bias whose exact gradient is zero.

Tolerances are NOT chosen here.  tools/text_encoder_errors.py measures, on the same inputs, what HF itself achieves on the
device against the fp64 values and writes profiles/text_encoder_errors.json; this file multiplies those figures:
  f32 mode   <= 4 x (HF fp32 on the GPU vs fp64)            -- the margin covers another summation order
  bf16 mode  <= 2 x (HF under bf16 autocast vs fp64)        -- the convention of the trunk's model tests
Recorded on an MI355X (profiles/text_encoder_errors.json; the HIP path's own figures are listed there for information only):
(worst parameter shown; the per-parameter figures are in the file)
  small  (hidden 64, 2 heads, 2 layers, B 3, L 37, lengths 37/20/1)
         hf_f32   out 1.9e-07  demb 2.4e-07  dparam 1.1e-06      hf_bf16  out 4.9e-04  demb 4.6e-04  dparam 1.1e-02
  base1  (hidden 768, 12 heads, 1 layer, B 2, L 128, lengths 128/77)
         hf_f32   out 6.5e-07  demb 7.7e-07  dparam 1.7e-05      hf_bf16  out 1.7e-03  demb 1.6e-03  dparam 3.0e-01
         (base1's worst parameter is attention.self.key.bias, whose exact gradient is zero: the floor's case)
Model level (mmtrvat at toy size, f32): text_encoder="hip" against "torch" on the same weights, bound = 4 x the larger
of (a) what HF-fp32-vs-HF-fp64 text features change in logits / gradients through the same trunk and (b) the torch path's
run-to-run figure: "model" entry of the same file (recorded: (a) logits 3.7e-07, gradients 2.4e-06; (b) 0 and 1.2e-07)."""
import copy
import json
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_FILE = os.path.join(ROOT, "profiles", "text_encoder_errors.json")
DEV = "cuda"
MARGIN = {"f32": 4.0, "bf16": 2.0}
HF_KEY = {"f32": "hf_f32", "bf16": "hf_bf16"}

CASES = {
    "small": dict(cfg=dict(vocab_size=60, hidden_size=64, num_attention_heads=2, num_hidden_layers=2, intermediate_size=256,
                           max_position_embeddings=64), B=3, L=37, lengths=[37, 20, 1]),
    "base1": dict(cfg=dict(vocab_size=60, hidden_size=768, num_attention_heads=12, num_hidden_layers=1, intermediate_size=3072,
                           max_position_embeddings=128), B=2, L=128, lengths=[128, 77]),
}


def recorded():
    assert os.path.exists(ERR_FILE), "profiles/text_encoder_errors.json is missing: python tools/text_encoder_errors.py on an MI355X"
    return json.load(open(ERR_FILE))


# ---------------------------------------------------------------------------------------------------------------------
# shared set-up (also used by tools/text_encoder_errors.py): one model, one input and one fp64 reference per case
# ---------------------------------------------------------------------------------------------------------------------
_CACHE = {}


def build(case, dropout=0.0):
    from transformers import BertConfig, BertModel
    c = CASES[case]
    torch.manual_seed(11)
    bert = BertModel(BertConfig(hidden_dropout_prob=dropout, attention_probs_dropout_prob=dropout, **c["cfg"]))
    with torch.no_grad():                       # HF initialises biases and LayerNorm affines to 0 / 1: make them count
        g = torch.Generator().manual_seed(12)
        for n, p in bert.named_parameters():
            if n.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "LayerNorm.weight" in n:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
    return bert


def inputs(case):
    c = CASES[case]
    B, L, d = c["B"], c["L"], c["cfg"]["hidden_size"]
    g = torch.Generator().manual_seed(13)
    ids = torch.randint(1, c["cfg"]["vocab_size"], (B, L), generator=g)
    mask = torch.zeros(B, L, dtype=torch.long)
    for b, n in enumerate(c["lengths"]):
        mask[b, :n] = 1
    ids = ids * mask                            # padded positions hold token 0
    seg = torch.zeros_like(ids)
    w = torch.randn(B, L, d, generator=g)       # the loss weights ALL positions, padded ones included
    return ids, mask, seg, w


def layer_grads(bert):
    return {n: p.grad.detach().double().cpu() for n, p in bert.named_parameters() if n.startswith("encoder.layer.")}


def run_hf(bert, ids, mask, seg, w, autocast=False):
    """HF forward + backward; returns {"out", "demb", "dparam": {name: grad}} as fp64 CPU tensors."""
    bert.zero_grad(set_to_none=True)
    kept = {}

    def hook(_m, _i, out):
        out.retain_grad()
        kept["emb"] = out

    h = bert.embeddings.register_forward_hook(hook)
    try:
        with torch.autocast("cuda", dtype=torch.bfloat16, enabled=autocast):
            out = bert(input_ids=ids, attention_mask=mask, token_type_ids=seg, return_dict=False)[0]
        (out.to(w.dtype) * w).sum().backward()
    finally:
        h.remove()
    return dict(out=out.detach().double().cpu(), demb=kept["emb"].grad.detach().double().cpu(), dparam=layer_grads(bert))


def run_hip(bert, ids, mask, seg, w, precision, seed=1, training=False, stack=None):
    from bpmult_amd.models.bert import BertLayerStack, run_layers
    bert.zero_grad(set_to_none=True)
    stack = stack or BertLayerStack(bert, precision)
    emb = bert.embeddings(input_ids=ids, token_type_ids=seg)
    emb.retain_grad()
    out = run_layers(stack, emb, mask, seed, training)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return dict(out=out.detach().double().cpu(), demb=emb.grad.detach().double().cpu(), dparam=layer_grads(bert))


def errors(got, ref):
    def e(a, b, floor=0.0):
        assert a.shape == b.shape and torch.isfinite(a).all()
        return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-300))
    floor = 1e-3 * max(float(t.abs().max()) for t in ref["dparam"].values())
    assert set(got["dparam"]) == set(ref["dparam"]) and len(ref["dparam"]) % 16 == 0
    per = {n: e(got["dparam"][n], ref["dparam"][n], floor) for n in ref["dparam"]}
    worst = max(per, key=per.get)
    return dict(out=e(got["out"], ref["out"]), demb=e(got["demb"], ref["demb"]), dparam=per[worst], worst_param=worst, per=per)


def check(got, rec, margin, what):
    """out, demb and EVERY parameter gradient against its own recorded HF figure times the margin"""
    bad = []
    for k in ("out", "demb"):
        if got[k] > margin * rec[k]:
            bad.append(f"{k}: {got[k]:.3e} > {margin:g} x {rec[k]:.3e}")
    assert set(got["per"]) == set(rec["per"])
    for n, v in got["per"].items():
        if v > margin * rec["per"][n]:
            bad.append(f"{n}: {v:.3e} > {margin:g} x {rec['per'][n]:.3e}")
    assert not bad, what + "\n  " + "\n  ".join(bad)


def brief(e):
    return {k: v for k, v in e.items() if k != "per"}


def reference(case):
    """(bert on the GPU (fp32, dropout 0, eval), device inputs, fp64 CPU reference) -- computed once, shared, never changed."""
    if case not in _CACHE:
        bert = build(case).eval()
        ids, mask, seg, w = inputs(case)
        ref = run_hf(copy.deepcopy(bert).double(), ids, mask, seg, w.double())
        _CACHE[case] = (bert.to(DEV), tuple(t.to(DEV) for t in (ids, mask, seg, w)), ref)
    return _CACHE[case]


# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("case", ["small", "base1"])
def test_layer_stack_matches_hf_fp64(case, precision):
    bert, dev_in, ref = reference(case)
    rec = recorded()[case]
    got = errors(run_hip(bert, *dev_in, precision), ref)
    hf = errors(run_hf(bert, *dev_in, autocast=precision == "bf16"), ref)          # re-measured here, printed, not used
    print(f"\n{case}/{precision}: hip {brief(got)}\n{case}/{precision}: hf  {brief(hf)}")
    for n in got["per"]:
        print(f"  {n:55s} hip {got['per'][n]:.3e}  recorded hf {rec[HF_KEY[precision]]['per'][n]:.3e}")
    check(got, rec[HF_KEY[precision]], MARGIN[precision], f"{case}/{precision}")


def test_bf16x3_runs_the_f32_path():
    bert, dev_in, ref = reference("small")
    a = run_hip(bert, *dev_in, "bf16x3")
    b = run_hip(bert, *dev_in, "f32")
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["demb"], b["demb"])


def test_train_mode_dropout():
    """HF's default dropout 0.1 on the probabilities and after both dense outputs: finite, different from eval, bit-equal
    for the same step seed, different for the next step's."""
    from bpmult_amd.models.bert import BertLayerStack
    bert = build("small", dropout=0.1).to(DEV).train()
    ids, mask, seg, w = (t.to(DEV) for t in inputs("small"))
    bert.embeddings.dropout.p = 0.0                 # torch's own generator drives this one: keep the embedding output fixed
    stack = BertLayerStack(bert, "bf16")
    ev = run_hip(bert, ids, mask, seg, w, "bf16", seed=5, training=False, stack=stack)
    a = run_hip(bert, ids, mask, seg, w, "bf16", seed=5, training=True, stack=stack)
    b = run_hip(bert, ids, mask, seg, w, "bf16", seed=5, training=True, stack=stack)
    c = run_hip(bert, ids, mask, seg, w, "bf16", seed=6, training=True, stack=stack)
    for r in (a, c):
        assert torch.isfinite(r["out"]).all() and torch.isfinite(r["demb"]).all()
        assert all(torch.isfinite(t).all() for t in r["dparam"].values())
    assert not torch.equal(a["out"], ev["out"]) and not torch.equal(a["demb"], ev["demb"])
    assert torch.equal(a["out"], b["out"]) and torch.equal(a["demb"], b["demb"])
    for n in a["dparam"]:
        assert torch.equal(a["dparam"][n], b["dparam"][n]), n
    assert not torch.equal(a["out"], c["out"]) and not torch.equal(a["demb"], c["demb"])
    # dropped elements are rescaled by 1 / 0.9, not lost: the train-mode output stays near the eval output
    assert float((a["out"] - ev["out"]).abs().mean()) < 0.5 * float(ev["out"].abs().mean())


def replay_fp64(bert64, ids, mask, seg, w, seed, p):
    """One training-mode pass of HF's layer arithmetic in fp64 on the CPU with the LIBRARY's dropout masks: the numpy
    restatement of the counter hash (test_kernels_gpu.drop_mult) at the sites and element indices models/bert.py
    documents -- probabilities: ((b*H + h)*L + i)*L + j; dense outputs: row (t*B + b), column c of [L*B, d]."""
    from bpmult_amd.models.bert import S_ATT_OUT, S_FFN_OUT, S_PROBS, bert_site
    from test_kernels_gpu import drop_mult
    F = torch.nn.functional
    cfg = bert64.config
    B, L = ids.shape
    d, H = cfg.hidden_size, cfg.num_attention_heads
    dh = d // H
    bert64.zero_grad(set_to_none=True)
    emb = bert64.embeddings(input_ids=ids, token_type_ids=seg)
    emb.retain_grad()
    hidden = (mask == 0)[:, None, None, :]

    def rowmask(site):          # [L*B, d] time-major rows -> [B, L, d]
        return drop_mult((L * B, d), p, seed, site).double().view(L, B, d).transpose(0, 1)

    x = emb
    for i, layer in enumerate(bert64.encoder.layer):
        a = layer.attention
        split = lambda t: t.view(B, L, H, dh).transpose(1, 2)
        q, k, v = split(a.self.query(x)), split(a.self.key(x)), split(a.self.value(x))
        sc = (q @ k.transpose(-1, -2)) * dh ** -0.5
        pr = torch.softmax(sc.masked_fill(hidden, float("-inf")), -1) * drop_mult((B, H, L, L), p, seed, bert_site(i, S_PROBS)).double()
        ctx = (pr @ v).transpose(1, 2).reshape(B, L, d)
        x1 = a.output.LayerNorm(a.output.dense(ctx) * rowmask(bert_site(i, S_ATT_OUT)) + x)
        g = F.gelu(layer.intermediate.dense(x1), approximate="none")
        x = layer.output.LayerNorm(layer.output.dense(g) * rowmask(bert_site(i, S_FFN_OUT)) + x1)
    (x * w).sum().backward()
    return dict(out=x.detach(), demb=emb.grad.detach(), dparam=layer_grads(bert64))


def test_backward_regenerates_the_forward_dropout_masks():
    """Train mode, f32: output AND gradients against an fp64 replay that applies the library's own masks (drawn on the host
    from the same counter hash) in forward only and lets autograd carry them into the backward.  A backward launch that
    regenerated another mask than the forward epilogue applied (LayerNorm backward's fused cast against the GEMM epilogue,
    dQ / dK-dV against the forward attention) would be wrong by whole elements here.  Bound: the f32 figures recorded for
    the same weights and inputs, per parameter."""
    p, seed = 0.1, 5
    bert = build("small", dropout=p).train()
    bert.embeddings.dropout.p = 0.0
    ids, mask, seg, w = inputs("small")
    ref = replay_fp64(copy.deepcopy(bert).double(), ids, mask, seg, w.double(), seed, p)
    bert = bert.to(DEV)
    got = errors(run_hip(bert, *(t.to(DEV) for t in (ids, mask, seg, w)), "f32", seed=seed, training=True), ref)
    print(f"\ndropout replay: hip f32 {brief(got)}")
    check(got, recorded()["small"]["hf_f32"], MARGIN["f32"], "dropout replay")


def test_encoder_module_draws_its_seed_from_the_step_counter(tmp_path):
    from bpmult_amd.models.bpmult import BertEncoder
    build("small", dropout=0.1).save_pretrained(tmp_path / "bert")
    args = SimpleNamespace(bert_model=str(tmp_path / "bert"), text_features=False, text_encoder="hip", precision="bf16")
    enc = BertEncoder(args).to(DEV).train()
    enc.bert.embeddings.dropout.p = 0.0
    ids, mask, seg, _ = (t.to(DEV) for t in inputs("small"))
    outs = []
    for step in (7, 7, 8):
        enc.dropout_step = step
        outs.append(enc(ids, mask, seg).detach().clone())
        assert enc.dropout_step == step + 1
    assert torch.equal(outs[0], outs[1]) and not torch.equal(outs[0], outs[2])
    enc.eval()
    with torch.no_grad():
        e1, e2 = enc(ids, mask, seg), enc(ids, mask, seg)
    assert torch.equal(e1, e2) and not torch.equal(e1, outs[0])
    # the same module under the default setting: HF's own forward, close to the HIP stack in eval mode
    args.text_encoder = "torch"
    ref = BertEncoder(args).to(DEV).eval()
    ref.load_state_dict(enc.state_dict())
    with torch.no_grad():
        r = ref(ids, mask, seg)
    rec = recorded()["small"]                        # the same weights and inputs as the "small" case
    tol = MARGIN["bf16"] * rec["hf_bf16"]["out"] + MARGIN["f32"] * rec["hf_f32"]["out"]
    assert float((r - e1).abs().max()) <= tol * float(r.abs().max())


# ---------------------------------------------------------------------------------------------------------------------
# model level
# ---------------------------------------------------------------------------------------------------------------------
def model_args(bert_dir, **kw):
    a = dict(model="mmtrvat", orig_d_l=64, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=24, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=2, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0., res_dropout=0.,
             out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6, bert_model=bert_dir, text_features=False,
             num_vectors_l=48, num_vectors_a=48, num_vectors_v=48, precision="f32")
    a.update(kw)
    return SimpleNamespace(**a)


def model_inputs():
    ids, mask, seg, _ = inputs("small")
    g = torch.Generator().manual_seed(21)
    B = ids.shape[0]
    img, aud = torch.randn(B, 40, 35, generator=g), torch.randn(B, 31, 74, generator=g)
    tgt = (torch.randn(B, 6, generator=g) > 0).float()
    return tuple(t.to(DEV) for t in (ids, mask, seg, img, aud, tgt))


def model_step(m, x):
    ids, mask, seg, img, aud, tgt = x
    m.zero_grad(set_to_none=True)
    logits = m(ids, mask, seg, img, aud)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt).backward()
    torch.cuda.synchronize()
    grads = {n: p.grad.detach().double().cpu() for n, p in m.named_parameters() if p.grad is not None}
    return dict(logits=logits.detach().double().cpu(), grads=grads)


def model_errors(got, ref):
    def e(a, b, floor=0.0):
        return float((a - b).abs().max() / max(float(b.abs().max()), floor, 1e-300))
    assert set(got["grads"]) == set(ref["grads"])
    floor = 1e-3 * max(float(t.abs().max()) for t in ref["grads"].values())
    per = {n: e(got["grads"][n], ref["grads"][n], floor) for n in ref["grads"]}
    worst = max(per, key=per.get)
    return dict(logits=e(got["logits"], ref["logits"]), grads=per[worst], worst_param=worst, per=per)


def model_check(got, rec, what):
    """logits and EVERY parameter gradient: 4 x the larger of the two recorded figures of that tensor"""
    a, b = rec["hf_f32_vs_f64_text"], rec["torch_run_to_run"]
    bad = []
    if got["logits"] > 4.0 * max(a["logits"], b["logits"]):
        bad.append(f"logits: {got['logits']:.3e} > 4 x {max(a['logits'], b['logits']):.3e}")
    assert set(got["per"]) == set(a["per"]) == set(b["per"])
    for n, v in got["per"].items():
        t = max(a["per"][n], b["per"][n])
        if v > 4.0 * t:
            bad.append(f"{n}: {v:.3e} > 4 x {t:.3e}")
    assert not bad, what + "\n  " + "\n  ".join(bad)


def build_models(tmp_path):
    """(hip model, torch model): same weights, eval-mode dropout-free BERT from a local directory, train mode trunk."""
    from bpmult_amd.models import get_model
    d = str(tmp_path / "bert")
    build("small").save_pretrained(d)
    torch.manual_seed(3)
    m_t = get_model(model_args(d))
    m_h = get_model(model_args(d, text_encoder="hip"))
    m_h.load_state_dict(m_t.state_dict())
    return m_h.to(DEV).train(), m_t.to(DEV).train()


def test_model_with_hip_text_encoder_matches_the_torch_text_encoder(tmp_path):
    rec = recorded()["model"]
    m_h, m_t = build_models(tmp_path)
    x = model_inputs()
    m_h.use_graphs = m_t.use_graphs = False
    ref = model_step(m_t, x)
    got = model_errors(model_step(m_h, x), ref)
    again = model_errors(model_step(m_t, x), ref)
    print(f"\nmodel: hip vs torch {brief(got)}\nmodel: torch vs torch {brief(again)}")
    assert any(n.startswith("enc.bert.encoder.layer.") for n in ref["grads"])
    model_check(got, rec, "model, hip against torch text encoder")


def test_trunk_graph_replay_still_engages_behind_the_hip_text_encoder(tmp_path):
    """use_graphs at its default: the text encoder runs as eager launches in front of the trunk's graphs, and the trunk's
    forward key is captured and replayed once it has recurred (two warm-up steps, then the capture)."""
    m_h, _ = build_models(tmp_path)
    x = model_inputs()
    outs = [model_step(m_h, x) for _ in range(4)]
    st = m_h._trunks[x[0].shape[0]].graph_stats
    assert st["captured"] >= 1 and st["failed"] == 0, st
    rec = recorded()["model"]
    got = model_errors(outs[3], outs[0])             # a replayed step against the first, eager one (same inputs, no dropout)
    model_check(got, rec, "replayed step against the eager one")
