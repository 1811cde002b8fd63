"""The BERT embeddings on the HIP path (`args.text_embeddings = "hip"`: bpm_bert_embed_fwd, bpm_bert_embed_scatter and
their host driver models/bert.py:BertEmbeddingsHip) on the MI355X against HF `BertEmbeddings` in fp64 on the CPU: the
output at ALL positions and the gradients of the five embedding parameters (word / position / type tables, LayerNorm
affine) under a loss that weights every position; then the module (`BertEncoder`) and the model with the HF layers behind.

Error measure of one tensor: max |got - ref| / max(max |ref|, floor), as in test_text_encoder_gpu.py; the floor (1e-3 of
the largest embedding-parameter gradient) only matters for a tensor whose exact gradient is zero.

Tolerances are NOT chosen here.  tools/text_embeddings_errors.py measures, on the same inputs, what HF's own fp32
embeddings achieve on the device against the fp64 values and writes profiles/text_embeddings_errors.json; every tensor is
held to 4 x ITS OWN recorded figure (the project's f32 margin for another summation order).  The embeddings produce
fp32 in every precision mode, so the same bound holds for the fp32 outputs under precision = "bf16"; the CT copy must be
BIT-EQUAL to what bpm_rows_cast makes of the fp32 output.

The embedding-level cases drive the host driver directly on a plan of its own (no layers behind it), so the figures are
those of the embedding kernels alone; the shapes are the smallest at which the kernels can still go wrong (see CASES).
Recorded on an MI355X (profiles/text_embeddings_errors.json; the HIP path's own figures are there for information only),
over all cases: hf_f32 0.4e-07 .. 4.3e-07 per tensor (dbeta of the one-row case exactly 0: one addend), the HIP path
0.5e-07 .. 2.0e-07 (and exactly 0 there as well; its output alone 0.5e-07 .. 1.0e-07: a row's LayerNorm is rounded once)."""
import copy
import json
import os
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ERR_FILE = os.path.join(ROOT, "profiles", "text_embeddings_errors.json")
DEV = "cuda"
MARGIN = 4.0
ULP = 2.0 ** -24
TENSORS = ("out", "dword", "dpos", "dtype", "dgamma", "dbeta")
GRAD_NAMES = dict(dword="word_embeddings.weight", dpos="position_embeddings.weight", dtype="token_type_embeddings.weight",
                  dgamma="LayerNorm.weight", dbeta="LayerNorm.bias")

# d, V, B, L, P -- what each covers
CASES = {
    "one_row": dict(d=32, V=7, B=1, L=1, P=4),            # one row, one 16-byte group per quarter wave
    "odd_rows": dict(d=64, V=60, B=3, L=37, P=64),        # R = 111: no multiple of the rows per block
    "full_pos": dict(d=64, V=60, B=3, L=64, P=64),        # L == P exactly
    "three_chunks": dict(d=768, V=60, B=2, L=128, P=128),  # three chunks per lane
    "widest": dict(d=1024, V=60, B=2, L=33, P=64),        # the widest instantiation
}
SEGS = ("zeros", "ones", "mixed")
TT = 2


def recorded():
    assert os.path.exists(ERR_FILE), "profiles/text_embeddings_errors.json is missing: python tools/text_embeddings_errors.py on an MI355X"
    return json.load(open(ERR_FILE))


# ---------------------------------------------------------------------------------------------------------------------
# shared set-up (also used by tools/text_embeddings_errors.py)
# ---------------------------------------------------------------------------------------------------------------------
def build_embeddings(case, padding_idx=0, dropout=0.0):
    """HF BertEmbeddings with every parameter random (HF zeroes the padding row and starts the affine at 1 / 0)."""
    from transformers import BertConfig
    from transformers.models.bert.modeling_bert import BertEmbeddings
    c = CASES[case]
    torch.manual_seed(31)
    cfg = BertConfig(vocab_size=c["V"], hidden_size=c["d"], max_position_embeddings=c["P"], type_vocab_size=TT, pad_token_id=padding_idx,
                     hidden_dropout_prob=dropout, num_attention_heads=1, num_hidden_layers=1, intermediate_size=32)
    emb = BertEmbeddings(cfg)
    assert emb.word_embeddings.padding_idx == padding_idx
    with torch.no_grad():
        g = torch.Generator().manual_seed(32)
        for n, p in emb.named_parameters():
            if n == "LayerNorm.weight":
                p.copy_(1.0 + 0.1 * torch.randn(p.shape, generator=g))
            else:
                p.copy_(0.1 * torch.randn(p.shape, generator=g) if n == "LayerNorm.bias" else torch.randn(p.shape, generator=g))
    return emb, cfg


def embed_inputs(case, seg_kind="mixed", ids_kind="random"):
    """ids never use token V - 2 (an id that does not occur -> an exactly zero gradient row) unless ids_kind says so"""
    c = CASES[case]
    B, L, V, d = c["B"], c["L"], c["V"], c["d"]
    g = torch.Generator().manual_seed(33)
    if ids_kind == "random":
        ids = torch.randint(0, V - 2, (B, L), generator=g)
        if B * L > 1:
            ids[-1, -1] = V - 1                                 # the last table row is used
            ids[0, 0] = 0                                       # so is the padding row's id
        else:
            ids[0, 0] = 3
    elif ids_kind == "same":
        ids = torch.full((B, L), 5)
    elif ids_kind == "distinct":
        ids = torch.randperm(V, generator=g)[:B * L].view(B, L)
    else:
        raise ValueError(ids_kind)
    seg = dict(zeros=torch.zeros(B, L, dtype=torch.long), ones=torch.ones(B, L, dtype=torch.long),
               mixed=(torch.arange(B * L).view(B, L) % 3 == 1).long())[seg_kind]
    w = torch.randn(B, L, d, generator=g)
    return ids, seg, w


def run_hf_embeddings(emb, ids, seg, w):
    """HF forward + backward -> {"out", "dword", ...} as fp64 CPU tensors"""
    emb.zero_grad(set_to_none=True)
    out = emb(input_ids=ids, token_type_ids=seg)
    (out * w).sum().backward()
    named = dict(emb.named_parameters())
    r = dict(out=out.detach().double().cpu())
    r.update({k: named[n].grad.detach().double().cpu() for k, n in GRAD_NAMES.items()})
    return r


class HipEmbeddings:
    """models/bert.py:BertEmbeddingsHip on a plan of its own: forward fills x[0] / xc[0], backward consumes a time-major
    gradient where it lies -- exactly the calls _EncoderFn makes, without layers in between."""

    def __init__(self, emb, cfg, B, L, precision="f32", tables=None):
        from bpmult_amd import config, ops
        from bpmult_amd.models.bert import BertEmbeddingsHip, _Plan
        d = cfg.hidden_size
        self.B, self.L, self.d = B, L, d
        self.st = SimpleNamespace(d=d, I=32, H=1, n_layers=1, device=torch.device(DEV, torch.cuda.current_device()),
                                  dtype=config.dtype_code(precision), ld=ops.pad32(d), ldI=32, dhp=32)
        self.pl = _Plan(self.st, B, L)
        self.bad = torch.zeros(1, device=DEV, dtype=torch.int32)
        self.drv = BertEmbeddingsHip(SimpleNamespace(config=cfg, embeddings=emb), self.bad)
        if tables is not None:                     # guarded views in place of the module's own tables
            self.drv.parameters = lambda: list(tables) + [emb.LayerNorm.weight, emb.LayerNorm.bias]

    def forward(self, ids, seg, seed=1, training=False):
        self.pl.seed, self.pl.training = seed, training
        self.drv.forward(self.st, self.pl, ids, seg, seed, training)
        return self.pl.x[0].view(self.L, self.B, self.d).transpose(0, 1)       # [B, L, d] view of the time-major rows

    def backward(self, w, need=(True,) * 5):
        self.pl.dx[0].view(self.L, self.B, self.d).copy_(w.transpose(0, 1))
        return self.drv.backward(self.st, self.pl, self.pl.dx[0], self.ids, self.seg, list(need))

    def run(self, ids, seg, w, seed=1, training=False):
        self.ids, self.seg = ids, seg
        out = self.forward(ids, seg, seed, training).detach().double().cpu()
        g = self.backward(w)
        torch.cuda.synchronize()
        r = dict(out=out)
        r.update({k: t.detach().double().cpu() for k, t in zip(("dword", "dpos", "dtype", "dgamma", "dbeta"), g)})
        return r


def errors(got, ref):
    floor = 1e-3 * max(float(ref[k].abs().max()) for k in TENSORS[1:])
    out = {}
    for k in TENSORS:
        a, b = got[k], ref[k]
        assert a.shape == b.shape and torch.isfinite(a).all(), k
        out[k] = float((a - b).abs().max() / max(float(b.abs().max()), floor if k != "out" else 0.0, 1e-300))
    return out


def check(got, rec, what):
    bad = [f"{k}: {got[k]:.3e} > {MARGIN:g} x {rec[k]:.3e}" for k in TENSORS if got[k] > MARGIN * rec[k]]
    assert not bad, what + "\n  " + "\n  ".join(bad)


_CACHE = {}


def reference(case, seg_kind="mixed", padding_idx=0, ids_kind="random"):
    """(embeddings on the GPU, cfg, device inputs, fp64 CPU reference) -- computed once, shared, never changed"""
    key = (case, seg_kind, padding_idx, ids_kind)
    if key not in _CACHE:
        emb, cfg = build_embeddings(case, padding_idx)
        emb.eval()
        ids, seg, w = embed_inputs(case, seg_kind, ids_kind)
        ref = run_hf_embeddings(copy.deepcopy(emb).double(), ids, seg, w.double())
        _CACHE[key] = (emb.to(DEV), cfg, tuple(t.to(DEV) for t in (ids, seg, w)), ref)
    return _CACHE[key]


def key_of(case, seg_kind, padding_idx, ids_kind="random"):
    return f"{case}/{seg_kind}/pad{padding_idx}/{ids_kind}"


# the combinations that are run (and recorded): every shape with mixed type ids and padding_idx 0; all-0 / all-1 type ids
# and padding_idx None on the multi-block small shape
COMBOS = [(c, "mixed", 0) for c in CASES] + [("odd_rows", "zeros", 0), ("odd_rows", "ones", 0), ("odd_rows", "mixed", None),
                                            ("three_chunks", "zeros", None)]
CASES["dup"] = dict(d=64, V=300, B=4, L=64, P=64)          # R = 256: eight 32-row pieces of one run (duplicates, below)
# everything tools/text_embeddings_errors.py records: (case, type ids, padding_idx, ids)
RECORDED = [c + ("random",) for c in COMBOS] + [("dup", "mixed", 0, "same"), ("dup", "mixed", 0, "distinct")]


def exact_zero_rows(case, seg_kind, padding_idx, ids, got):
    """rows that no input touches, and the padding row, are EXACTLY zero"""
    c = CASES[case]
    used = torch.zeros(c["V"], dtype=torch.bool)
    used[ids.cpu().view(-1)] = True
    if padding_idx is not None:
        used[padding_idx] = False
    assert (~used).any()
    assert torch.equal(got["dword"][~used], torch.zeros_like(got["dword"][~used]))
    assert got["dword"][used].abs().sum(1).min() > 0
    if c["L"] < c["P"]:
        assert torch.equal(got["dpos"][c["L"]:], torch.zeros_like(got["dpos"][c["L"]:]))
    for tt, absent in ((0, seg_kind == "ones"), (1, seg_kind == "zeros" or c["B"] * c["L"] == 1)):
        if absent:
            assert torch.equal(got["dtype"][tt], torch.zeros_like(got["dtype"][tt]))


# ---------------------------------------------------------------------------------------------------------------------
# 1. forward and backward against fp64
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("precision", ["f32", "bf16"])
@pytest.mark.parametrize("case,seg_kind,padding_idx", COMBOS)
def test_embeddings_match_hf_fp64(case, seg_kind, padding_idx, precision):
    from bpmult_amd import ops
    emb, cfg, (ids, seg, w), ref = reference(case, seg_kind, padding_idx)
    c = CASES[case]
    h = HipEmbeddings(emb, cfg, c["B"], c["L"], precision)
    got = h.run(ids, seg, w)
    e = errors(got, ref)
    rec = recorded()[key_of(case, seg_kind, padding_idx)]["hf_f32"]
    print(f"\n{key_of(case, seg_kind, padding_idx)}/{precision}: hip {e}\n  recorded hf_f32 {rec}")
    check(e, rec, f"{case}/{seg_kind}/{padding_idx}/{precision}")
    exact_zero_rows(case, seg_kind, padding_idx, ids, got)
    assert int(h.bad) == 0
    # the CT copy: bit-equal to what bpm_rows_cast makes of the fp32 output
    R, d, ld = c["B"] * c["L"], c["d"], h.st.ld
    xc = torch.full_like(h.pl.xc[0], 7.0)
    ops.rows_cast(h.st.dtype, [ops.cast_problem(h.pl.x[0], d, R, d, dst_ct=xc, ldd=ld)], 0)
    assert torch.equal(xc, h.pl.xc[0])
    # mean / rstd / s are those of the pre-LayerNorm sum
    s = h.pl.s.double()
    assert torch.allclose(h.pl.emean.double(), s.mean(1), rtol=0, atol=1e-5 * float(s.abs().max()))
    assert torch.allclose(h.pl.erstd.double(), (s.var(1, unbiased=False) + cfg.layer_norm_eps).rsqrt(), rtol=1e-5, atol=0)


# ---------------------------------------------------------------------------------------------------------------------
# 2. duplicates: one id in all R = 256 rows (chunked runs), every id distinct, the last id
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("ids_kind", ["same", "distinct"])
def test_duplicate_and_distinct_ids(ids_kind):
    emb, cfg, (ids, seg, w), ref = reference("dup", "mixed", 0, ids_kind)
    got = HipEmbeddings(emb, cfg, 4, 64).run(ids, seg, w)
    e = errors(got, ref)
    rec = recorded()[key_of("dup", "mixed", 0, ids_kind)]["hf_f32"]
    print(f"\ndup/{ids_kind}: hip {e}\n  recorded hf_f32 {rec}")
    check(e, rec, f"dup/{ids_kind}")
    exact_zero_rows("dup", "mixed", 0, ids, got)
    if ids_kind == "same":
        assert int((got["dword"].abs().sum(1) > 0).sum()) == 1


def test_runs_that_straddle_chunks_and_the_last_id():
    """Sorted runs of 1 .. 70 rows laid so that they start, end and continue at every offset of a 32-position chunk; the
    longest run belongs to id V - 1.  Reference: the same sums in fp64 (index_add), bound: 4 x one fp32 rounding per
    addend of the longest run -- (n - 1) 2^-24 relative to the sum of absolute values, the textbook bound of a
    sequential fp32 sum (Higham, Accuracy and Stability of Numerical Algorithms, eq. 4.4)."""
    from bpmult_amd import ops
    B, L, d, V = 4, 64, 64, 40
    R = B * L
    g = torch.Generator().manual_seed(41)
    lens, ids = [1, 31, 33, 2, 64, 5, 27, 23], []
    lens.append(R - sum(lens))                                      # 70 rows of id V - 1
    for n, tok in zip(lens, [3, 4, 7, 9, 12, 20, 21, 30, V - 1]):
        ids += [tok] * n
    ids = torch.tensor(ids)[torch.randperm(R, generator=g)].view(B, L).to(DEV)
    ds = torch.randn(R, d, generator=g).to(DEV)
    dword = torch.zeros(V, d, device=DEV)
    sid, perm = torch.sort(ids.view(-1), stable=True)
    ws = torch.empty(ops.bert_embed_scatter_ws_bytes(R, d, 0) // 4, device=DEV)
    ops.bert_embed_scatter(ops.bert_scatter_problem(ds, B, L, ws, sorted_ids=sid, perm=perm, dword=dword, padding_idx=None), d)
    rows = (torch.arange(L).view(1, L) * B + torch.arange(B).view(B, 1)).view(-1).to(DEV)      # batch-major position -> time-major row
    ref = torch.zeros(V, d, dtype=torch.float64, device=DEV).index_add_(0, ids.view(-1), ds[rows].double())
    mag = torch.zeros(V, d, dtype=torch.float64, device=DEV).index_add_(0, ids.view(-1), ds[rows].double().abs())
    torch.cuda.synchronize()
    assert bool(((dword.double() - ref).abs() <= MARGIN * (max(lens) - 1) * ULP * mag).all())
    assert int((dword.abs().sum(1) > 0).sum()) == len(lens)


# ---------------------------------------------------------------------------------------------------------------------
# 3. bit-reproducibility
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("case", ["odd_rows", "three_chunks", "dup"])
def test_gradients_are_bit_reproducible(case):
    emb, cfg, (ids, seg, w), _ = reference(case, "mixed", 0, "same" if case == "dup" else "random")
    c = CASES[case]
    h = HipEmbeddings(emb, cfg, c["B"], c["L"])
    a = h.run(ids, seg, w)
    b = h.run(ids, seg, w)
    for k in TENSORS:
        assert torch.equal(a[k], b[k]), k


# ---------------------------------------------------------------------------------------------------------------------
# 4. dropout
# ---------------------------------------------------------------------------------------------------------------------
def test_dropout_uses_the_keyed_hash_in_forward_and_backward():
    """Training, p = 0.1: the output is the eval output times the host-side mask of site bert_site(0, S_EMBED) in
    time-major element order; the backward against an fp64 replay of HF's arithmetic with that mask applied in forward only
    (autograd carries it into the backward), within the f32 bounds recorded for the same weights and inputs; another step
    seed draws another mask."""
    from bpmult_amd.models.bert import S_EMBED, bert_site
    from test_kernels_gpu import drop_mult
    case, p, seed = "odd_rows", 0.1, 5
    emb, cfg = build_embeddings(case, 0, dropout=p)
    ids, seg, w = embed_inputs(case)
    c = CASES[case]
    B, L, d = c["B"], c["L"], c["d"]
    mask = drop_mult((L * B, d), p, seed, bert_site(0, S_EMBED)).double().view(L, B, d).transpose(0, 1)
    e64 = copy.deepcopy(emb).double().eval()
    out = e64(input_ids=ids, token_type_ids=seg) * mask
    (out * w.double()).sum().backward()
    named = dict(e64.named_parameters())
    ref = dict(out=out.detach())
    ref.update({k: named[n].grad.detach() for k, n in GRAD_NAMES.items()})
    emb = emb.to(DEV).train()
    ids, seg, w = (t.to(DEV) for t in (ids, seg, w))
    h = HipEmbeddings(emb, cfg, B, L)
    ev = h.forward(ids, seg, seed, training=False).detach().cpu().clone()
    got = h.run(ids, seg, w, seed=seed, training=True)
    assert 0.05 < float((mask == 0).double().mean()) < 0.15
    want = ev.double() * mask                                          # one fp32 multiply by 0 or by fp32(1 / 0.9)
    assert torch.equal(got["out"][mask == 0], want[mask == 0]) and bool(((got["out"] - want).abs() <= 4 * ULP * want.abs()).all())
    e = errors(got, ref)
    rec = recorded()[key_of(case, "mixed", 0)]["hf_f32"]
    print(f"\ndropout replay: hip {e}\n  recorded hf_f32 {rec}")
    check(e, rec, "dropout replay")
    other = h.forward(ids, seg, seed + 1, training=True).detach().cpu()
    assert not torch.equal(other.double(), got["out"])


# ---------------------------------------------------------------------------------------------------------------------
# 5. bounds without risk
# ---------------------------------------------------------------------------------------------------------------------
def test_ids_outside_a_table_give_zero_rows_and_are_counted():
    """Every table is a view into a larger buffer with one guard row of 1e30 in front and one behind: a read outside the
    table stays inside memory this test owns and would show the sentinel."""
    case = "odd_rows"
    emb, cfg = build_embeddings(case, 0)
    emb = emb.to(DEV).eval()
    c = CASES[case]
    B, L, V, d = c["B"], c["L"], c["V"], c["d"]
    ids, seg, w = (t.to(DEV) for t in embed_inputs(case))

    def guarded(t):
        buf = torch.full((t.shape[0] + 2, t.shape[1]), 1e30, device=DEV)
        buf[1:-1] = t.detach()
        return buf[1:-1]

    tables = [guarded(emb.word_embeddings.weight), guarded(emb.position_embeddings.weight), guarded(emb.token_type_embeddings.weight)]
    h = HipEmbeddings(emb, cfg, B, L, tables=tables)
    bad_ids, bad_seg = ids.clone(), seg.clone()
    bad_ids[0, 3], bad_ids[1, 7], bad_ids[2, L - 1] = -1, V, V + 1000
    bad_seg[1, 2], bad_seg[0, 3] = TT, -5                             # [0, 3]: both ids of one position are bad
    got = h.run(bad_ids, bad_seg, w)
    assert int(h.bad) == 5
    assert torch.isfinite(got["out"]).all() and float(got["out"].abs().max()) < 1e3
    # the expected result: the same kernels on word / type tables with a ZERO row in front and one behind, every id moved
    # up by one, ids below the table pointing at the front row and ids beyond it at the back row -- bit for bit: the
    # sorted list keeps its layout (bad ids sort to the same ends), so every sum keeps its order and its pieces
    zrow = torch.zeros(1, d, device=DEV)
    longer = [torch.cat([zrow, t.detach(), zrow]) for t in (emb.word_embeddings.weight, emb.token_type_embeddings.weight)]
    h2 = HipEmbeddings(emb, cfg, B, L, tables=[longer[0], emb.position_embeddings.weight.detach(), longer[1]])
    h2.drv.padding_idx = 1
    ok_ids = torch.where(bad_ids < 0, torch.zeros_like(bad_ids), torch.where(bad_ids >= V, torch.full_like(bad_ids, V + 1), bad_ids + 1))
    ok_seg = torch.where(bad_seg < 0, torch.zeros_like(bad_seg), torch.where(bad_seg >= TT, torch.full_like(bad_seg, TT + 1), bad_seg + 1))
    ref = h2.run(ok_ids, ok_seg, w)
    assert int(h2.bad) == 0
    ref["dword"], ref["dtype"] = ref["dword"][1:V + 1], ref["dtype"][1:TT + 1]
    for k in TENSORS:
        assert torch.equal(got[k], ref[k]), k
    rows = torch.tensor([3 * B + 0, 7 * B + 1])                       # time-major rows of the positions with a bad word id and a good type id
    assert float(got["out"].transpose(0, 1).reshape(L * B, d)[rows].abs().max()) < 1e3
    for t in tables:                                                  # the guard rows were not written either
        base = t._base if t._base is not None else t
        assert torch.equal(base[0], torch.full_like(base[0], 1e30)) and torch.equal(base[-1], torch.full_like(base[-1], 1e30))


# ---------------------------------------------------------------------------------------------------------------------
# 6. module and model
# ---------------------------------------------------------------------------------------------------------------------
def _encoders(tmp_path, precision="f32"):
    import test_text_encoder_gpu as T
    from bpmult_amd.models.bpmult import BertEncoder
    T.build("small").save_pretrained(tmp_path / "bert")
    mk = lambda **kw: BertEncoder(SimpleNamespace(bert_model=str(tmp_path / "bert"), text_features=False, text_encoder="hip",
                                                  precision=precision, **kw)).to(DEV).eval()
    enc_t, enc_h = mk(), mk(text_embeddings="hip")
    enc_h.load_state_dict(enc_t.state_dict())
    return enc_t, enc_h


def _enc_step(enc, ids, mask, seg, w):
    enc.zero_grad(set_to_none=True)
    out = enc(ids, mask, seg)
    (out * w).sum().backward()
    torch.cuda.synchronize()
    return out.detach().double().cpu(), {n: (p.grad.detach().double().cpu() if p.grad is not None else None)
                                         for n, p in enc.bert.named_parameters() if not n.startswith("pooler.")}


def test_encoder_module_hip_embeddings_against_torch_embeddings(tmp_path):
    """BertEncoder, text_encoder = "hip", f32, eval: text_embeddings "hip" against "torch" on the same weights -- the hidden
    state and EVERY BERT parameter gradient.  Bounds: 4 x the HF-fp32-against-fp64 figure of that tensor on these weights
    and inputs: layer parameters and the hidden state from profiles/text_encoder_errors.json ("small"), the embedding
    parameters from the "small_encoder" entry of profiles/text_embeddings_errors.json (their gradients THROUGH the layers)."""
    import test_text_encoder_gpu as T
    enc_t, enc_h = _encoders(tmp_path)
    ids, mask, seg, w = (t.to(DEV) for t in T.inputs("small"))
    o_t, g_t = _enc_step(enc_t, ids, mask, seg, w)
    o_h, g_h = _enc_step(enc_h, ids, mask, seg, w)
    rec_l = T.recorded()["small"]["hf_f32"]
    rec_e = recorded()["small_encoder"]["hf_f32"]
    floor = 1e-3 * max(float(t.abs().max()) for t in g_t.values())
    rel = lambda a, b, fl=0.0: float((a - b).abs().max() / max(float(b.abs().max()), fl, 1e-300))
    bad = []
    if rel(o_h, o_t) > MARGIN * rec_l["out"]:
        bad.append(f"out: {rel(o_h, o_t):.3e} > 4 x {rec_l['out']:.3e}")
    assert set(g_h) == set(g_t) and all(v is not None for v in g_h.values())
    for n in g_t:
        bound = rec_e[n] if n.startswith("embeddings.") else rec_l["per"][n]
        e = rel(g_h[n], g_t[n], floor)
        print(f"  {n:55s} hip-vs-torch embeddings {e:.3e}  recorded hf {bound:.3e}")
        if e > MARGIN * bound:
            bad.append(f"{n}: {e:.3e} > 4 x {bound:.3e}")
    assert not bad, "\n  ".join(bad)
    assert int(enc_h.bad_token_ids) == 0 and enc_t.bad_token_ids is None
    # segment=None means all zeros
    with torch.no_grad():
        assert torch.equal(enc_h(ids, mask, None), enc_h(ids, mask, torch.zeros_like(ids)))


def test_encoder_module_bf16_and_frozen_embeddings(tmp_path):
    """precision = "bf16": the embeddings stay fp32, so the first layer input is bit-equal to the f32 mode's; frozen
    embeddings give None gradients, the same output and the same layer gradients."""
    import test_text_encoder_gpu as T
    _, enc = _encoders(tmp_path, "bf16")
    ids, mask, seg, w = (t.to(DEV) for t in T.inputs("small"))
    o1, g1 = _enc_step(enc, ids, mask, seg, w)
    x0_bf16 = enc._stack._plans[tuple(ids.shape)].x[0].clone()
    enc.bert.embeddings.requires_grad_(False)
    o2, g2 = _enc_step(enc, ids, mask, seg, w)
    assert torch.equal(o1, o2)
    for n in g1:
        if n.startswith("embeddings."):
            assert g1[n] is not None and g2[n] is None, n
        else:
            assert torch.equal(g1[n], g2[n]), n
    enc.precision = "f32"
    with torch.no_grad():
        enc(ids, mask, seg)
    assert torch.equal(enc._stack._plans[tuple(ids.shape)].x[0], x0_bf16)


def _models(tmp_path):
    import test_text_encoder_gpu as T
    from bpmult_amd.models import get_model
    d = str(tmp_path / "bert")
    T.build("small").save_pretrained(d)
    torch.manual_seed(3)
    m_t = get_model(T.model_args(d, text_encoder="hip"))
    m_h = get_model(T.model_args(d, text_encoder="hip", text_embeddings="hip"))
    m_h.load_state_dict(m_t.state_dict())
    return m_h.to(DEV).train(), m_t.to(DEV).train()


def test_model_with_hip_embeddings_matches_the_torch_embeddings_model(tmp_path):
    """mmtrvat at toy size, f32, text_encoder = "hip" in both models: logits and EVERY parameter gradient of the
    text_embeddings = "hip" model against the "torch"-embeddings model, within the recorded "model" bound of
    profiles/text_encoder_errors.json (4 x the larger of HF-fp32-vs-fp64 text features through the same trunk and the torch
    path's run-to-run figure, per tensor).

    Measured on an MI355X: logits 2.108e-07 (bound 4 x 3.689e-07); the largest ratio of a gradient to its recorded figure
    is 3.56 (trans_l_with_a.layers.1.layer_norms.1.weight), then 2.67 and 2.5.  The two models differ only in the first layer
    input, two evaluations of the same embeddings; the HIP one rounds a row's LayerNorm once (fp64 registers), so what is
    left is the torch kernel's own fp32 noise.  (With fp32 statistics in the HIP kernel as well, the two noises added up to
    4.000008 x the figure of trans_a_with_l.layers.0.fc1.weight: over the bound.)"""
    import test_text_encoder_gpu as T
    m_h, m_t = _models(tmp_path)
    x = T.model_inputs()
    m_h.use_graphs = m_t.use_graphs = False
    ref = T.model_step(m_t, x)
    got = T.model_errors(T.model_step(m_h, x), ref)
    print(f"\nmodel: hip embeddings vs torch embeddings {T.brief(got)}")
    assert any(n.startswith("enc.bert.embeddings.") for n in ref["grads"])
    T.model_check(got, T.recorded()["model"], "model, hip against torch embeddings")
    assert int(m_h.enc.bad_token_ids) == 0


def test_trunk_graph_replay_still_engages_behind_the_hip_embeddings(tmp_path):
    import test_text_encoder_gpu as T
    m_h, _ = _models(tmp_path)
    x = T.model_inputs()
    outs = [T.model_step(m_h, x) for _ in range(4)]
    st = m_h._trunks[x[0].shape[0]].graph_stats
    assert st["captured"] >= 1 and st["failed"] == 0, st
    T.model_check(T.model_errors(outs[3], outs[0]), T.recorded()["model"], "replayed step against the eager one")
