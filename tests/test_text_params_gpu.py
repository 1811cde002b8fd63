"""`args.text_params = "flat"` on the MI355X: the text encoder's parameters in a flat store of their own, their gradients
written there by the HIP backward, and FusedAdam stepping trunk + text in ONE launch (bpm_adam_step_sets).

Kernel level, on GIVEN gradients (test_optim_groups_gpu.flat_grads): one set is bit-equal to bpm_adam_step_groups, two
sets are bit-equal to two one-set launches that read the same counters, text parameters hold the project's kernel limit
(max-abs 2e-6, test_optim_groups_gpu.LIMIT) against torch.optim.Adam / AdamW over four steps at lr <= 3e-3.
Model level: "flat" against "torch" on the same weights and inputs -- gradients, accumulation micro-steps, one optimizer
step, a skipped step, the global norm, checkpoints in both directions and a foreign optimizer.

Bit comparisons are made only where the two modes run the same launches without float atomics (weight matrices, the
three embedding tables, logits); biases and LayerNorm affines are summed with float atomics and are held against the
fp64 HF reference with the bound tests/test_text_encoder_gpu.py applies to that tensor.  For that the gradient tests (e),
(f) run the "small" case of that file (the weights and inputs its recorded figures belong to); the others run the tiny
BERT (hidden 32, 2 layers, B 2, L 12, one padded sample) behind the toy trunk."""
import copy
import hashlib

import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import _lib, engine, ops  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.models.bert import _WEIGHTS, EMBED_PARAMS, build_text_store  # noqa: E402
from bpmult_amd.optim import FusedAdam, grad_norm  # noqa: E402
from test_optim_groups_gpu import LIMIT, flat_grads, toy  # noqa: E402

DEV = "cuda"
TINY = dict(vocab_size=60, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64, max_position_embeddings=32)
HYPER = [dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, decoupled_weight_decay=False),
         dict(lr=1e-3, betas=(0.8, 0.999), eps=1e-8, weight_decay=0.1, decoupled_weight_decay=True),
         dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False)]


def sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().view(torch.uint8).numpy().tobytes()).hexdigest()


def tiny_bert():
    from transformers import BertConfig, BertModel
    torch.manual_seed(11)
    bert = BertModel(BertConfig(hidden_dropout_prob=0.0, attention_probs_dropout_prob=0.0, **TINY))
    with torch.no_grad():                       # as test_text_encoder_gpu.build: biases and LayerNorm affines that count
        g = torch.Generator().manual_seed(12)
        for n, p in bert.named_parameters():
            if n.endswith(".bias"):
                p.copy_(0.1 * torch.randn(p.shape, generator=g))
            elif "LayerNorm.weight" in n:
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
    return bert


def group_of(st, out=()):
    """L2 / decoupled / vectors, as test_optim_groups_gpu.test_groups_against_torch: vectors 2, matrices alternate 0 / 1."""
    g, k = {}, 0
    for n in st.names:
        if n in out:
            continue
        if st.params[n].ndim <= 1:
            g[n] = 2
        else:
            g[n] = k & 1
            k += 1
    return g


class Bench:
    """One store with start values and moments to restore, and what a launch leaves."""

    def __init__(self, st, seed):
        self.st = st
        st.refresh_shadows(force=True)
        g = torch.Generator().manual_seed(seed)
        self.master0, self.shadow0 = st.master.clone(), st.shadow_flat.clone()
        self.m0 = (torch.randn(st.total, generator=g) * 1e-2).to(DEV)
        self.v0 = (torch.rand(st.total, generator=g) * 1e-4).to(DEV)
        self.grads = [flat_grads(st, seed + 1 + i)[0] for i in range(4)]
        self.m, self.v = self.m0.clone(), self.v0.clone()

    def reset(self, grad=0):
        self.st.master.copy_(self.master0)
        self.st.shadow_flat.copy_(self.shadow0)
        self.st.gflat.copy_(self.grads[grad])
        self.m.copy_(self.m0)
        self.v.copy_(self.v0)
        self.st._dirty, self.st._shadow_sig = False, self.st._versions()

    def state(self):
        return [t.clone() for t in (self.st.master, self.m, self.v, self.st.shadow_flat, self.st.gflat)]

    def buffers(self):
        return (self.st.master, self.st.gflat, self.m, self.v)


WHAT = ("master", "exp_avg", "exp_avg_sq", "shadows", "gradients")


@pytest.fixture(scope="module", params=["f32", "bf16"])
def stores(request):
    """Hidden-40 trunk store (column and parameter padding) and the tiny text store, one CT for both."""
    torch.manual_seed(3)
    m = toy(hidden=40, num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    m.precision = request.param
    m = m.cuda()
    trunk = m._ensure_store()
    bert = tiny_bert().to(DEV)
    text = build_text_store(bert, trunk.dtype, True, "enc.")
    assert trunk.shadow_flat.dtype == text.shadow_flat.dtype == (torch.bfloat16 if request.param == "bf16" else torch.float32)
    return m, bert, Bench(trunk, 40), Bench(text, 60)


def dev_args(case):
    """(scale_dev, norm_dev, steps_dev, skipped_dev) of a case; fresh tensors every call"""
    f = lambda x: torch.tensor([x], device=DEV, dtype=torch.float32)
    steps = lambda: torch.tensor([1, 7, 3, 0], device=DEV, dtype=torch.int32)
    skipped = lambda: torch.tensor([5], device=DEV, dtype=torch.int32)
    return {"host_steps": (None, None, None, None), "scale_dev": (f(0.37), None, None, None),
            "norm_finite": (f(0.37), f(2.5), steps(), skipped()), "norm_nan": (None, f(float("nan")), steps(), skipped()),
            "norm_inf_no_steps": (None, f(float("inf")), None, skipped())}[case]


CASES = ("host_steps", "scale_dev", "norm_finite", "norm_nan", "norm_inf_no_steps")


def launch_sets(benches, group_ofs, case, zero_grad, step=2):
    sts = [b.st for b in benches]
    table = engine.adam_sets_table(sts, group_ofs)
    sets = ops.adam_sets([b.buffers() for b in benches])
    scale, norm, steps, skipped = dev_args(case)
    engine.adam_step_sets(sts, table, sets, ops.adam_groups([dict(h, step=step) for h in HYPER]), 0.5, zero_grad, scale_dev=scale,
                          norm_dev=norm, steps_dev=steps, skipped_dev=skipped)
    return table, steps, skipped


# ---------------------------------------------------------------------------------------------------------------------
# (a) one set == bpm_adam_step_groups
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("which", ["trunk", "text"])
def test_one_set_is_bit_equal_to_step_groups(stores, which):
    """L2 and decoupled groups, the vectors' group, two parameters in no group (-1 segments), scale_dev, norm_dev finite
    and NaN / inf with steps_dev / skipped_dev, with and without zero_grad: master, both moments, shadows and the
    (cleared) gradients carry the same SHA-256 as bpm_adam_step_groups leaves on the same start values."""
    b = stores[2] if which == "trunk" else stores[3]
    st = b.st
    out = [n for n in st.names if n in st._adam_plain][:1] + [n for n in st.names if st.params[n].ndim == 1][:1]
    g = group_of(st, out)
    assert len(out) == 2 and set(g.values()) == {0, 1, 2}
    for case in CASES:
        for zero_grad in (False, True):
            b.reset()
            scale, norm, steps, skipped = dev_args(case)
            st.adam_step_groups(b.m, b.v, st.adam_group_table(g), ops.adam_groups([dict(h, step=2) for h in HYPER]), 0.5, zero_grad,
                                scale_dev=scale, norm_dev=norm, steps_dev=steps, skipped_dev=skipped)
            want, wc = b.state(), (steps, skipped)
            b.reset()
            table, steps, skipped = launch_sets([b], [g], case, zero_grad)
            got = b.state()
            for a, c, what in zip(want, got, WHAT):
                assert sha256(a) == sha256(c), (case, zero_grad, what)
            for a, c in zip(wc, (steps, skipped)):
                assert (a is None and c is None) or torch.equal(a, c), (case, "counters")
            skipped_step = case in ("norm_nan", "norm_inf_no_steps")
            assert torch.equal(got[0], b.master0) == skipped_step and torch.equal(got[3], b.shadow0) == skipped_step
            assert (float(got[4].abs().max()) == 0.0) == zero_grad
            for n in out:                                                      # not stepped: bits kept
                a, e = st.off[n], st.off[n] + st.params[n].numel()
                assert torch.equal(got[0][a:e], b.master0[a:e]) and torch.equal(got[1][a:e], b.m0[a:e])
    b.reset()


# ---------------------------------------------------------------------------------------------------------------------
# (b) two sets == two one-set launches
# ---------------------------------------------------------------------------------------------------------------------
def test_two_sets_are_bit_equal_to_two_one_set_launches(stores):
    _, _, trunk, text = stores
    gs = [group_of(trunk.st, [n for n in trunk.st.names if n in trunk.st._adam_plain][:1]), group_of(text.st)]
    for case in CASES:
        want = []
        for b, g in zip((trunk, text), gs):                                    # each reads the same (fresh) counters
            b.reset()
            _, steps, skipped = launch_sets([b], [g], case, True)
            want.append((b.state(), steps, skipped))
        trunk.reset()
        text.reset()
        table, steps, skipped = launch_sets([trunk, text], gs, case, True)
        for b, (state, s1, k1) in zip((trunk, text), want):
            for a, c, what in zip(state, b.state(), WHAT):
                assert sha256(a) == sha256(c), (case, what)
            assert (s1 is None and steps is None) or torch.equal(s1, steps), case
            assert torch.equal(k1, skipped) if k1 is not None else skipped is None, case
        if case == "norm_finite":
            assert steps.tolist() == [2, 8, 4, 0] and skipped.tolist() == [5]     # exactly one per group of the launch
        if case == "norm_nan":
            assert steps.tolist() == [1, 7, 3, 0] and skipped.tolist() == [6]     # exactly one skip, no count moved
        if case == "norm_inf_no_steps":
            assert skipped.tolist() == [6]
    # the table holds what the comparison is meant to cover
    host, nseg = table[1], table[2]
    chunk = 4 * 256                                                              # f32x4 per block (bpm_adam_blocks(chunk) == 1)
    assert ops.adam_blocks(chunk) == 1 and ops.adam_blocks(chunk + 1) == 2
    assert any(sg.n4 < chunk for sg in host), "no segment shorter than one block"
    last = {}
    for sg in host:
        last[(sg.group & 0xffffffff) >> _lib.ADAM_SET_SHIFT] = sg
    assert set(last) == {0, 1} and any(sg.n4 % chunk for sg in last.values()), "no set whose last block is partial"
    assert any((sg.group & 0xff) == 0xff for sg in host) and any(sg.dst for sg in host)
    trunk.reset()
    text.reset()


# ---------------------------------------------------------------------------------------------------------------------
# (c) text parameters against torch
# ---------------------------------------------------------------------------------------------------------------------
def test_text_parameters_against_torch_adam(stores):
    """Four steps of the two-set launch on given gradients against torch.optim.Adam over clones with the same groups (group 1
    decoupled: AdamW); one text matrix and one text vector in no group keep master, moments and shadow bits."""
    _, _, trunk, text = stores
    st = text.st
    frozen = ["enc.bert.encoder.layer.1.intermediate.dense.weight", "enc.bert.encoder.layer.0.attention.output.LayerNorm.bias"]
    gs = [group_of(trunk.st), group_of(st, frozen)]
    trunk.reset()
    text.reset()
    text.m.zero_()
    text.v.zero_()
    trunk.m.zero_()
    trunk.v.zero_()
    ref = {n: st.params[n].detach().clone().requires_grad_(True) for n in gs[1]}
    opt = torch.optim.Adam([dict(h, params=[ref[n] for n in gs[1] if gs[1][n] == i]) for i, h in enumerate(HYPER)])
    table = engine.adam_sets_table([trunk.st, st], gs)
    sets = ops.adam_sets([trunk.buffers(), text.buffers()])
    for it in range(1, 5):
        trunk.st.gflat.copy_(trunk.grads[it - 1])
        st.gflat.copy_(text.grads[it - 1])
        for n, r in ref.items():
            r.grad = st.g(n).clone()
        opt.step()
        engine.adam_step_sets([trunk.st, st], table, sets, ops.adam_groups([dict(h, step=it) for h in HYPER]), 1.0, False)
        d = torch.stack([(st.params[n].detach() - r.detach()).abs().max() for n, r in ref.items()])
        i = int(d.argmax())
        print("step", it, "worst text parameter", float(d[i]), list(ref)[i])
        assert float(d[i]) <= LIMIT, (it, float(d[i]), list(ref)[i])
    assert not torch.equal(st.master, text.master0)
    for n in frozen:
        a, e = st.off[n], st.off[n] + (st.params[n].numel() + 63) // 64 * 64
        assert torch.equal(st.master[a:e], text.master0[a:e]), n
        assert float(text.m[a:e].abs().max()) == 0.0 and float(text.v[a:e].abs().max()) == 0.0, n
    rows, cols, dst_ld, off = st._adam_plain[frozen[0]]
    assert torch.equal(st.shadow_flat[off: off + rows * dst_ld], text.shadow0[off: off + rows * dst_ld])
    # every other shadow is the CT image of its updated master
    got = st.shadow_flat.clone()
    st.refresh_shadows(force=True)
    assert torch.equal(got, st.shadow_flat)
    trunk.reset()
    text.reset()


# ---------------------------------------------------------------------------------------------------------------------
# (d) argument errors
# ---------------------------------------------------------------------------------------------------------------------
def test_argument_errors_launch_nothing(stores):
    _, _, trunk, text = stores
    trunk.reset()
    text.reset()
    sts = [trunk.st, text.st]
    gs = [group_of(trunk.st), group_of(text.st)]
    tab, host, nseg, nblk = engine.adam_sets_table(sts, gs)
    sets_dev, sets_host, _ = ops.adam_sets([trunk.buffers(), text.buffers()])
    groups = ops.adam_groups([dict(h, step=1) for h in HYPER])
    before = [sha256(t) for b in (trunk, text) for t in b.state()]
    L, ARG, ALIGN = _lib.lib(), -1, -2
    stream = torch.cuda.current_stream().cuda_stream

    def call(table_dev=tab.data_ptr(), table_host=host, nseg=nseg, nblk=nblk, sdev=sets_dev.data_ptr(), shost=sets_host, nsets=2,
             groups=groups, ngroups=3, scale=None, steps=None):
        return L.bpm_adam_step_sets(trunk.st.dtype, table_dev, table_host, nseg, nblk, sdev, shost, nsets, groups, ngroups, 1.0, scale,
                                    None, steps, None, 1, stream)

    assert call(table_dev=None) == ARG and call(table_host=None) == ARG
    assert call(sdev=None) == ARG and call(shost=None) == ARG
    assert call(groups=None) == ARG
    assert call(nsets=0) == ARG and call(nsets=5) == ARG
    assert call(nsets=1) == ARG                                                   # segments of set 1, one set
    assert call(ngroups=0) == ARG and call(ngroups=17) == ARG
    assert call(groups=ops.adam_groups([dict(h, step=0) for h in HYPER])) == ARG  # host step < 1 without steps_dev
    assert call(nblk=nblk - 1) == ARG and call(nseg=nseg - 1) == ARG              # blocks that do not add up
    short = (_lib.AdamSet * 2)(*sets_host)
    short[1].n = text.st.total - 64                                               # the last text segment now reaches beyond its set
    assert call(shost=short) == ARG
    odd = (_lib.AdamSet * 2)(*sets_host)
    odd[0].exp_avg += 4
    assert call(shost=odd) == ALIGN
    assert call(scale=trunk.m.data_ptr() + 2) == ALIGN and call(steps=trunk.m.data_ptr() + 1) == ALIGN
    torch.cuda.synchronize()
    assert [sha256(t) for b in (trunk, text) for t in b.state()] == before        # nothing was launched


# ---------------------------------------------------------------------------------------------------------------------
# (e), (f): gradients, "flat" against "torch", on the "small" case of test_text_encoder_gpu.py
# ---------------------------------------------------------------------------------------------------------------------
def _encoders(tmp_path, precision="f32", embeddings="hip"):
    import test_text_encoder_gpu as T
    from types import SimpleNamespace
    from bpmult_amd.models.bpmult import BertEncoder
    T.build("small").save_pretrained(tmp_path / "bert")
    mk = lambda **kw: BertEncoder(SimpleNamespace(bert_model=str(tmp_path / "bert"), text_features=False, text_encoder="hip",
                                                  text_embeddings=embeddings, precision=precision, **kw)).to(DEV).eval()
    enc_t, enc_f = mk(), mk(text_params="flat")
    enc_f.load_state_dict(enc_t.state_dict())
    return enc_t, enc_f


def _enc_backward(enc, ids, mask, seg, w):
    out = enc(ids, mask, seg)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach()


def _is_matrix(n):
    return n.endswith(tuple(_WEIGHTS)) or n.endswith(EMBED_PARAMS[:3])


def test_gradients_flat_against_torch(tmp_path):
    import test_text_embeddings_gpu as E
    import test_text_encoder_gpu as T
    enc_t, enc_f = _encoders(tmp_path)
    ids, mask, seg, w = (t.to(DEV) for t in T.inputs("small"))
    o_t, o_f = _enc_backward(enc_t, ids, mask, seg, w), _enc_backward(enc_f, ids, mask, seg, w)
    assert torch.equal(o_t, o_f)                                                  # the same launches on the same weights
    st = enc_f.flat_store()
    lo, hi = st.gflat.data_ptr(), st.gflat.data_ptr() + 4 * st.total
    g_t = {n: p.grad for n, p in enc_t.bert.named_parameters() if not n.startswith("pooler.")}
    g_f = {n: p.grad for n, p in enc_f.bert.named_parameters() if not n.startswith("pooler.")}
    assert len(g_f) == 2 * 16 + 5 and all(g is not None for g in g_f.values())
    assert all(p.grad is None for n, p in enc_f.bert.named_parameters() if n.startswith("pooler."))
    # fp64 reference of the same weights and inputs (HF on the CPU), embedding affine included
    ref64 = copy.deepcopy(T.build("small").eval()).double()
    ri, rm, rs, rw = T.inputs("small")
    (ref64(input_ids=ri, attention_mask=rm, token_type_ids=rs, return_dict=False)[0] * rw.double()).sum().backward()
    ref = {n: p.grad for n, p in ref64.named_parameters() if not n.startswith("pooler.")}
    rec_l = T.recorded()["small"]["hf_f32"]["per"]
    rec_e = E.recorded()["small_encoder"]["hf_f32"]
    floor = 1e-3 * max(float(t.abs().max()) for n, t in ref.items() if n.startswith("encoder.layer."))
    bad = []
    for n, g in g_f.items():
        assert lo <= g.data_ptr() and g.data_ptr() + 4 * g.numel() <= hi, n      # .grad IS the store's view
        assert g.data_ptr() == st.g("bert." + n).data_ptr(), n
        if _is_matrix(n):
            assert torch.equal(g, g_t[n]), n                                      # same launches, no float atomics
        else:
            bound = T.MARGIN["f32"] * (rec_e[n] if n.startswith("embeddings.") else rec_l[n])
            e = float((g.double().cpu() - ref[n]).abs().max() / max(float(ref[n].abs().max()), floor, 1e-300))
            print(f"  {n:55s} flat vs fp64 {e:.3e}  bound {bound:.3e}")
            if e > bound:
                bad.append(f"{n}: {e:.3e} > {bound:.3e}")
    assert not bad, "\n  ".join(bad)


def test_flat_layers_behind_torch_embeddings(tmp_path):
    """text_embeddings = "torch": the store holds the layers only; the embeddings stay PyTorch's and get their gradients from
    autograd, through the embedding-output gradient the stack hands back.  Two micro-steps: outputs and layer matrices
    bit-equal to the "torch" mode; the embedding parameters' gradients lie outside the store and agree (torch sums the
    table rows with float atomics: no bit comparison, 1e-5 of the tensor's largest element)."""
    import test_text_encoder_gpu as T
    enc_t, enc_f = _encoders(tmp_path, embeddings="torch")
    ids, mask, seg, w = (t.to(DEV) for t in T.inputs("small"))
    outs = {}
    for enc in (enc_t, enc_f):
        outs[enc] = [_enc_backward(enc, ids, mask, seg, w), _enc_backward(enc, ids, torch.ones_like(mask), seg, 0.5 * w)]
    assert all(torch.equal(a, b) for a, b in zip(outs[enc_t], outs[enc_f]))
    st = enc_f.flat_store()
    assert st.names[0].startswith("bert.encoder.layer.1.") and not any("embeddings" in n for n in st.names)
    lo, hi = st.gflat.data_ptr(), st.gflat.data_ptr() + 4 * st.total
    g_t = dict(enc_t.bert.named_parameters())
    for n, p in enc_f.bert.named_parameters():
        if n.startswith("pooler."):
            continue
        assert (lo <= p.grad.data_ptr() < hi) == n.startswith("encoder.layer."), n
        if n.startswith("embeddings."):
            assert float((p.grad - g_t[n].grad).abs().max()) <= 1e-5 * float(g_t[n].grad.abs().max()), n
        elif _is_matrix(n):
            assert torch.equal(p.grad, g_t[n].grad), n


def test_two_accumulation_micro_steps(tmp_path):
    """Two micro-steps on different inputs without clearing in between: "flat" (F_ACCUM launches; the embedding tables
    through the scratch copy and one bpm_add_n) against "torch" (autograd's `+=` of two fresh gradients).  Embedding tables
    and weight matrices bit-equal: the F_ACCUM epilogue adds the finished fp32 product to what lies there, one fp32 add
    per element like autograd's."""
    import test_text_encoder_gpu as T
    enc_t, enc_f = _encoders(tmp_path)
    ids, mask, seg, w = (t.to(DEV) for t in T.inputs("small"))
    g = torch.Generator().manual_seed(77)
    ids2 = (torch.randint(1, 60, ids.shape, generator=g).to(DEV)) * mask.flip(0)
    mask2, w2 = mask.flip(0).contiguous(), torch.randn(w.shape, generator=g).to(DEV)
    for enc in (enc_t, enc_f):
        _enc_backward(enc, ids, mask, seg, w)
        _enc_backward(enc, ids2, mask2, seg, w2)
    g_t = {n: p.grad for n, p in enc_t.bert.named_parameters() if not n.startswith("pooler.")}
    g_f = {n: p.grad for n, p in enc_f.bert.named_parameters() if not n.startswith("pooler.")}
    single = _encoders(tmp_path)[1]
    _enc_backward(single, ids2, mask2, seg, w2)
    ulp = 2.0 ** -23
    for n in g_f:
        if not _is_matrix(n):
            continue
        d = float((g_f[n] - g_t[n]).abs().max())
        print(f"  {n:55s} max-abs difference {d:.3e} at magnitude {float(g_t[n].abs().max()):.3e}")
        assert not torch.equal(g_f[n], dict(single.bert.named_parameters())[n].grad), n       # it did accumulate
        if n.startswith("embeddings."):
            assert torch.equal(g_f[n], g_t[n]), n
        else:
            assert d <= ulp * float(g_t[n].abs().max()), n                       # expected 0; never more than one ulp at the max
            assert torch.equal(g_f[n], g_t[n]), n


# ---------------------------------------------------------------------------------------------------------------------
# model level: tiny BERT behind the toy trunk
# ---------------------------------------------------------------------------------------------------------------------
@pytest.fixture(scope="module")
def tiny_dir(tmp_path_factory):
    d = str(tmp_path_factory.mktemp("tiny") / "bert")
    tiny_bert().save_pretrained(d)
    return d


def make_models(d, precision="f32", modes=("flat", "torch")):
    import test_text_encoder_gpu as T
    torch.manual_seed(3)
    ms = [get_model(T.model_args(d, orig_d_l=32, text_encoder="hip", text_embeddings="hip", text_params=mode, precision=precision))
          for mode in modes]
    for m in ms[1:]:
        m.load_state_dict(ms[0].state_dict())
    for m in ms:
        m.to(DEV).train()
        m.use_graphs = False
    return ms


def model_inputs(seed=21):
    g = torch.Generator().manual_seed(seed)
    ids = torch.randint(1, 60, (2, 12), generator=g)
    mask = torch.ones(2, 12, dtype=torch.long)
    mask[1, 7:] = 0                                                               # one padded sample
    ids = ids * mask
    img, aud = torch.randn(2, 40, 35, generator=g), torch.randn(2, 31, 74, generator=g)
    tgt = (torch.randn(2, 6, generator=g) > 0).float()
    return tuple(t.to(DEV) for t in (ids, mask, torch.zeros_like(ids), img, aud, tgt))


def backward(m, x):
    ids, mask, seg, img, aud, tgt = x
    logits = m(ids, mask, seg, img, aud)
    torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt).backward()
    return logits.detach()


def text_matrices(m):
    return {n: p for n, p in m.named_parameters() if n.startswith("enc.bert.") and _is_matrix(n)}


def count_packs(fn):
    """Runs fn with ops.pack_weights wrapped: the device tables of the pack launches it issued."""
    seen, real = [], ops.pack_weights
    ops.pack_weights = lambda dtype, table, *a: (seen.append(table.data_ptr()), real(dtype, table, *a))[1]
    try:
        out = fn()
    finally:
        ops.pack_weights = real
    return seen, out


def check_step_and_shadows(d, precision):
    m_f, m_t = make_models(d, precision)
    x = model_inputs()
    o_f, o_t = backward(m_f, x), backward(m_t, x)
    assert torch.equal(o_f, o_t)
    opts = [FusedAdam(m, lr=1e-3) for m in (m_f, m_t)]
    for o in opts:
        o.step()
    torch.cuda.synchronize()
    text = m_f.enc.flat_store()
    assert m_f._flat_stores() == [m_f._store, text] and m_t._flat_stores() == [m_t._store]
    tail = [opts[0]._name_of[id(p)] for tg in opts[0]._tail_opt.param_groups for p in tg["params"]]
    assert not any(n.startswith(("enc.bert.encoder.", "enc.bert.embeddings.")) for n in tail), tail
    assert any(n.startswith("enc.bert.pooler.") for n in tail)
    t_tail = [opts[1]._name_of[id(p)] for tg in opts[1]._tail_opt.param_groups for p in tg["params"]]
    assert any(n.startswith("enc.bert.encoder.") for n in t_tail)
    named_t = dict(m_t.named_parameters())
    mats = text_matrices(m_f)
    assert len(mats) == 2 * 6 + 3
    for n, p in mats.items():                                                     # weight matrices and the three tables
        e = float((p.detach() - named_t[n].detach()).abs().max())
        assert e <= LIMIT, (n, e)
    # every text shadow == pack_weights of the updated masters (packed into a scratch copy of the shadows)
    got = text.shadow_flat.clone()
    text.shadow_flat.zero_()
    ops.pack_weights(text.dtype, *text._table)
    torch.cuda.synchronize()
    assert torch.equal(got, text.shadow_flat) and float(got.float().abs().max()) > 0
    assert got.dtype == (torch.bfloat16 if precision == "bf16" else torch.float32)
    # the next forward packs nothing for the text store (and the trunk only its rest table)
    text_tables = {t[0].data_ptr() for t in (text._table, text._rest_table) if t is not None}
    seen, _ = count_packs(lambda: backward(m_f, x))
    assert not text_tables & set(seen), "the text store's shadows were re-packed after a fused step"
    seen_t, _ = count_packs(lambda: backward(m_t, x))
    assert len(seen_t) == len(seen) + 1                                            # "torch" mode: the stack's own re-pack


def test_one_step_both_modes_f32(tiny_dir):
    check_step_and_shadows(tiny_dir, "f32")


def test_one_step_both_modes_bf16(tiny_dir):
    check_step_and_shadows(tiny_dir, "bf16")


def snapshot(m, opt):
    opt._store()
    out = [t.clone() for st in m._flat_stores() for t in (st.master, st.shadow_flat)] + [t.clone() for t in opt._ms + opt._vs]
    for n, p in m.named_parameters():
        if not any(n in st.params for st in m._flat_stores()):
            out.append(p.detach().clone())
    return out


def test_skip_nonfinite_with_one_text_gradient_inf(tiny_dir):
    (m,) = make_models(tiny_dir, modes=("flat",))
    x = model_inputs()
    backward(m, x)
    torch.cuda.synchronize()
    trunk, text = m._flat_stores()
    given = [trunk.gflat.clone(), text.gflat.clone()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    opt = FusedAdam(m, lr=1e-3, skip_nonfinite=True, param_groups=[
        dict(params=[p for p in m.parameters() if p.ndim >= 2], weight_decay=0.01), dict(params=[p for p in m.parameters() if p.ndim < 2])])
    before = snapshot(m, opt)
    k = text.off["enc.bert.encoder.layer.0.intermediate.dense.weight"] + 5
    text.gflat[k] = float("inf")
    opt.step()
    assert all(torch.equal(a, b) for a, b in zip(before, snapshot(m, opt)))       # no master, moment, shadow or tail parameter
    assert opt._counters[:2].tolist() == [0, 0] and int(opt.skipped_steps) == 1
    assert not bool(torch.isfinite(opt.last_grad_norm))
    text.gflat.copy_(given[1])
    opt.step()                                                                    # the clean step ...
    after = snapshot(m, opt)
    assert opt._counters[:2].tolist() == [1, 1] and int(opt.skipped_steps) == 1
    with torch.no_grad():
        for n, p in m.named_parameters():
            p.copy_(start[n])
    first = FusedAdam(m, lr=1e-3, skip_nonfinite=True, param_groups=[
        dict(params=[p for p in m.parameters() if p.ndim >= 2], weight_decay=0.01), dict(params=[p for p in m.parameters() if p.ndim < 2])])
    trunk.gflat.copy_(given[0])
    text.gflat.copy_(given[1])
    for p, g in zip([p for p in m.parameters() if p.grad is not None], given[2:]):
        p.grad.copy_(g)
    first.step()                                                                  # ... equals a first step
    want = snapshot(m, first)
    assert len(want) == len(after) and all(torch.equal(a, b) for a, b in zip(want, after))
    assert not torch.equal(after[0], before[0]) and not torch.equal(after[2], before[2])


def test_global_norm_over_both_stores_and_the_tail(tiny_dir):
    (m,) = make_models(tiny_dir, modes=("flat",))
    backward(m, model_inputs())
    torch.cuda.synchronize()
    want = float(torch.sqrt(sum(p.grad.double().square().sum() for p in m.parameters() if p.grad is not None)))
    text_sq = float(sum(p.grad.double().square().sum() for n, p in m.named_parameters() if n.startswith("enc.bert.e")))
    assert text_sq > 1e-3 * want ** 2                                             # the text share counts
    bound = 14 * 2.0 ** -24                                                       # 13 * 2^-24 + one fp32 rounding (bpm_grad_sumsq)
    a, b = grad_norm(m), grad_norm(m)
    print("grad_norm", float(a), "fp64", want, "relative error", abs(float(a) - want) / want, "bound", bound)
    assert torch.equal(a, b)
    assert abs(float(a) - want) <= bound * want
    start = {n: p.detach().clone() for n, p in m.named_parameters()}
    master0 = [st.master.clone() for st in m._flat_stores()]
    given = [st.gflat.clone() for st in m._flat_stores()] + [p.grad.clone() for p in m.parameters() if p.grad is not None]
    res = []
    for _ in range(2):
        with torch.no_grad():
            for n, p in m.named_parameters():
                p.copy_(start[n])
        for st, g in zip(m._flat_stores(), given):
            st.gflat.copy_(g)
        for p, g in zip([p for p in m.parameters() if p.grad is not None], given[2:]):
            p.grad.copy_(g)
        opt = FusedAdam(m, lr=1e-3, max_grad_norm=0.5 * want)
        opt.step()
        res.append([opt.last_grad_norm.clone()] + snapshot(m, opt))
    assert abs(float(res[0][0]) - want) <= bound * want
    assert all(torch.equal(a, b) for a, b in zip(*res))                           # two runs, bit-equal
    assert all(not torch.equal(st.master, m0) for st, m0 in zip(m._flat_stores(), master0))       # (the step ran, in both stores)


def test_state_dict_round_trip_and_switching_at_a_resume(tiny_dir):
    m_f, m_t, m_r = make_models(tiny_dir, modes=("flat", "torch", "flat"))
    x1, x2 = model_inputs(21), model_inputs(22)
    o_f, o_t, o_r = (FusedAdam(m, lr=1e-3, weight_decay=0.01) for m in (m_f, m_t, m_r))
    for m, o in ((m_f, o_f), (m_t, o_t)):
        backward(m, x1)
        o.step()
        o.zero_grad()
    sd_f, sd_t = copy.deepcopy(o_f.state_dict()), copy.deepcopy(o_t.state_dict())
    text = m_f.enc.flat_store()
    assert set(sd_f["flat_text"]) == {"exp_avg", "exp_avg_sq", "names", "offsets"} and "flat_text" not in sd_t
    assert sd_f["flat_text"]["names"] == text.names and float(sd_f["flat_text"]["exp_avg"].abs().max()) > 0
    # round trip: a fresh "flat" model + optimizer continue like the uninterrupted one
    m_r.load_state_dict(m_f.state_dict())
    o_r.load_state_dict(sd_f)
    assert torch.equal(o_r._ms[1], o_f._ms[1]) and torch.equal(o_r._vs[1], o_f._vs[1]) and torch.equal(o_r._m, o_f._m)
    assert o_r.state_dict()["group_steps"] == [1]
    # a "torch" checkpoint into a "flat" optimizer: the per-parameter moments of its tail state land in the flat text moments
    (m_s,) = make_models(tiny_dir, modes=("flat",))
    o_s = FusedAdam(m_s, lr=1e-3, weight_decay=0.01)
    m_s.load_state_dict(m_f.state_dict())                                         # (after copying the masters)
    o_s.load_state_dict(sd_t)
    st_s = m_s.enc.flat_store()
    named_t = dict(m_t.named_parameters())
    for n in st_s.names:
        a, k = st_s.off[n], st_s.params[n].numel()
        assert torch.equal(o_s._ms[1][a:a + k], o_t._tail_opt.state[named_t[n]]["exp_avg"].reshape(-1)), n
        assert torch.equal(o_s._vs[1][a:a + k], o_t._tail_opt.state[named_t[n]]["exp_avg_sq"].reshape(-1)), n
    tail_s = [o_s._name_of[id(p)] for tg in o_s._tail_opt.param_groups for p in tg["params"]]
    assert not any(n in st_s.params for n in tail_s) and "out_layer.weight" in tail_s
    assert torch.equal(o_s._tail_opt.state[m_s.out_layer.weight]["exp_avg"], o_t._tail_opt.state[m_t.out_layer.weight]["exp_avg"])
    o_s._ms[1].copy_(o_f._ms[1])                                                  # "from equal moments"
    o_s._vs[1].copy_(o_f._vs[1])
    o_s._m.copy_(o_f._m)
    o_s._v.copy_(o_f._v)
    for m, o in ((m_f, o_f), (m_s, o_s), (m_r, o_r)):
        backward(m, x2)
        o.step()
    torch.cuda.synchronize()
    # Every matrix and table of the model.  The vectors are left out: their gradients are sums of float atomics that differ
    # from run to run in the last bits, and where the exact gradient is zero (a key bias shifts every score of a row alike)
    # Adam's normalisation turns that noise into updates of +-lr -- in either mode, between any two runs.
    named_f = dict(m_f.named_parameters())
    for other in (m_s, m_r):
        for n, p in other.named_parameters():
            if p.ndim >= 2:
                e = float((p.detach() - named_f[n].detach()).abs().max())
                assert e <= LIMIT, (n, e)
    # the reverse direction says so
    with pytest.raises(ValueError, match="text_params='flat'.*not supported"):
        o_t.load_state_dict(sd_f)


def test_a_foreign_optimizer_still_repacks(tiny_dir):
    """A plain torch.optim.Adam(model.parameters()) on a "flat" model trains two steps; the forward then reads re-packed
    shadows (the version counters), as a "torch"-mode model with the same weights shows."""
    m_f, m_t = make_models(tiny_dir)
    x = model_inputs()
    opt = torch.optim.Adam(m_f.parameters(), lr=1e-3)
    for _ in range(2):
        opt.zero_grad(set_to_none=False)
        backward(m_f, x)
        opt.step()
    m_t.load_state_dict(m_f.state_dict())
    text = m_f.enc.flat_store()
    assert text.still_flat()
    with torch.no_grad():
        seen, a = count_packs(lambda: m_f(*x[:5]))
        b = m_t(*x[:5])
    assert text._table[0].data_ptr() in seen
    assert torch.equal(a, b)
    # raw `p.data` writers: invalidate_shadows() keeps working
    with torch.no_grad():
        m_f.enc.bert.encoder.layer[0].output.dense.weight.data.mul_(1.5)
        m_f.enc.invalidate_shadows()
        m_t.load_state_dict(m_f.state_dict())
        assert torch.equal(m_f(*x[:5]), m_t(*x[:5]))
