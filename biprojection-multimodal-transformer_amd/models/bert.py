"""The layer stack of an HF `BertModel` on the HIP path (reference mmtr.py:144-158: the text encoder upstream of the
trunk; opt-in through `args.text_encoder = "hip"`, models/bpmult.py:BertEncoder).

The module tree stays HF's: parameters, `state_dict` keys and optimizer groups are untouched.  `BertLayerStack` only
reads `bert.encoder.layer[*]` and runs the post-LN layers as grouped launches behind ONE autograd node (`_StackFn`):
embedding output [B, L, d] + attention mask [B, L] + the layers' parameters in, last hidden state [B, L, d] out; backward
returns the gradient of the embedding output and of every layer parameter.  The embeddings (a gather + LayerNorm) run on
torch by default; with `args.text_embeddings = "hip"` they are HIP kernels too (`BertEmbeddingsHip` below) and the node
becomes `_EncoderFn`: (ids, type ids, byte mask, embedding parameters, layer parameters) -> last hidden state.  The pooler
is not evaluated (the reference discards its output).

Schedule of one layer, rows time-major (row = t*B + b, what the head-major attention layout expects), x fp32 [R, d]:

  xc            = CT(x)                                                      bpm_rows_cast
  q, k, v       = heads(xc Wq^T + bq) dh^-0.5, heads(xc Wk^T + bk), ..       bpm_gemm_grouped NT, BPM_OUT_HEADS (one launch)
  ctx, lse      = softmax(q k^T | key mask) v, dropout on the probabilities  bpm_attn_fwd_kmask
  y1            = drop(ctx Wo^T + bo) + x                                    NT, bias -> dropout -> + resid epilogue
  x1            = LN(y1), x1c = CT(x1)                                       bpm_ln_fwd (fp32 out), bpm_rows_cast
  u             = x1c Wi^T + bi                                              NT, BPM_OUT_CT
  g             = gelu(u)                                                    bpm_gelu_fwd
  y2            = drop(g Wo2^T + bo2) + x1                                   NT, bias -> dropout -> + resid epilogue
  x'            = LN(y2)                                                     bpm_ln_fwd

Backward mirrors it: bpm_ln_bwd_ws (whose fused cast output is d(dense output) = dropmask(dy) as CT, with the dense bias
gradient as its column sums), TN weight gradients (colsum_a for the q / k / v / intermediate biases), NN data gradients
(the residual gradient rides in their `resid` epilogue), bpm_gelu_bwd, bpm_attn_bwd_dq_kmask / _dkv_kmask.

Key mask: HF's `attention_mask` as bytes [B, L], built on the device ((mask != 0).to(uint8)); no length ever travels to
the host.  Padded QUERY positions are computed like any other (HF does, and the trunk consumes them).  Every sample needs
at least one visible key.

Embeddings on the HIP path (HF `BertEmbeddings`, absolute positions):

  x, xc, s, mean, rstd = drop(LN((word[id] + type[seg]) + pos[t]))          bpm_bert_embed_fwd: writes the plan's x[0] and
                                                                             xc[0] in time-major rows straight from the
                                                                             batch-major int64 ids (no cast, no transpose)
  backward, from the stack's dx buffer (time-major, consumed where it lies):
  g             = dy * dropmask                                              bpm_rows_cast (training with p > 0 only)
  ds, dgamma, dbeta = dLN(g | s, mean, rstd)                                 bpm_ln_bwd_ws (the deterministic workspace route)
  dword, dpos, dtype                                                         bpm_bert_embed_scatter (two launches, no float
                                                                             atomics: bit-reproducible), after a stable
                                                                             torch.sort of the ids on the device
  The existing rows_cast + ln_bwd_ws pair was preferred to one fused new kernel: it costs one launch more in training and
  none in eval, and reuses the workspace reduction that is already tested.  fp32 tensors in every precision mode (the forward carries a row's LayerNorm in fp64 registers and rounds once).

Parameters (`args.text_params`): "torch" (the default) leaves them PyTorch's -- backward returns fresh gradient tensors
to autograd, an optimizer steps them one by one and the next forward re-packs the CT shadows.  "flat" (build_text_store):
the layer parameters (and the HIP embeddings') are views into an engine.ParamStore; the backward launches write the
store's gradient buffer under the trunk's rules (unset gradients: the weight-gradient GEMMs store and one
bpm_zero_segments launch clears the rest; otherwise F_ACCUM, and the embedding tables through a scratch copy + bpm_add_n),
the nodes return None for the stored parameters, every finished section (layer n-1 ... 0, then the embeddings) is
reported to `grad_ready`, and the shadows belong to the store, where FusedAdam's kernel writes them.

Precision: "bf16" = bf16 MFMA operands (CT shadows of the weights, refreshed when a parameter's version changes), fp32
accumulation, fp32 residual stream and LayerNorm; "f32" = exact fp32 products; "bf16x3" runs this stack's f32 path.
"""
from __future__ import annotations

from typing import Dict, List, Optional, Tuple

import torch

from .. import config, ops
from .._lib import F_ACCUM, F_KPAD, GEMM_NN, GEMM_NT, GEMM_TN, OUT_CT, OUT_F32, OUT_HEADS, PackDesc
from ..engine import ParamStore, dhp_for
from ..ops import pad32

# dropout sites of the text encoder: disjoint from engine.site() (enc_id < 12 -> below 1 << 16) and engine.SITE_TEXT (1 << 20)
SITE_BERT = 1 << 21
S_PROBS, S_ATT_OUT, S_FFN_OUT = range(3)
S_EMBED = 3                      # bert_site(0, S_EMBED): the embedding output's dropout, element (t*B + b)*d + c
MAX_EMBED_HIDDEN = 1024          # reach of the 16-byte row kernels (one wave per row, four chunks per lane)

# per layer, in this order (HF names below bert.encoder.layer[i])
LAYER_PARAMS = ("attention.self.query.weight", "attention.self.query.bias", "attention.self.key.weight", "attention.self.key.bias",
                "attention.self.value.weight", "attention.self.value.bias", "attention.output.dense.weight",
                "attention.output.dense.bias", "attention.output.LayerNorm.weight", "attention.output.LayerNorm.bias",
                "intermediate.dense.weight", "intermediate.dense.bias", "output.dense.weight", "output.dense.bias",
                "output.LayerNorm.weight", "output.LayerNorm.bias")
_WEIGHTS = ("attention.self.query.weight", "attention.self.key.weight", "attention.self.value.weight",
            "attention.output.dense.weight", "intermediate.dense.weight", "output.dense.weight")


def bert_site(layer: int, op: int) -> int:
    return SITE_BERT | (layer << 4) | op


def check_config(cfg) -> None:
    """What the HIP layer stack implements; anything else is refused when the model is built."""
    act = getattr(cfg, "hidden_act", "gelu")
    if act != "gelu":
        raise ValueError(f"text_encoder='hip': hidden_act {act!r} is not supported (only the exact erf 'gelu')")
    pet = getattr(cfg, "position_embedding_type", "absolute")
    if pet != "absolute":
        raise ValueError(f"text_encoder='hip': position_embedding_type {pet!r} is not supported (only 'absolute')")
    if getattr(cfg, "is_decoder", False) or getattr(cfg, "add_cross_attention", False):
        raise ValueError("text_encoder='hip': is_decoder / add_cross_attention are not supported (a bidirectional encoder only)")
    if cfg.hidden_size % cfg.num_attention_heads:
        raise ValueError("text_encoder='hip': hidden_size must be divisible by num_attention_heads")
    dh = cfg.hidden_size // cfg.num_attention_heads
    if dh > 256:
        raise ValueError(f"text_encoder='hip': head_dim {dh} > 256 is not supported by the attention kernels")
    if cfg.hidden_size % 32 or cfg.intermediate_size % 32:
        raise ValueError("text_encoder='hip': hidden_size and intermediate_size must be multiples of 32 (rows without padding "
                         f"columns; got {cfg.hidden_size} / {cfg.intermediate_size}): other sizes are not covered by a parity test yet")


def layer_parameters(bert) -> List[torch.nn.Parameter]:
    """The stack's parameters in the order _StackFn takes them and returns their gradients."""
    out = []
    for layer in bert.encoder.layer:
        named = dict(layer.named_parameters())
        out += [named[n] for n in LAYER_PARAMS]
    return out


def build_text_store(bert, dtype: int, embeddings: bool, prefix: str = "") -> ParamStore:
    """The flat store of the text parameters whose gradients the HIP path produces (`args.text_params = "flat"`): the 16
    LAYER_PARAMS of every layer and, with `embeddings`, the five EMBED_PARAMS, re-pointed into one fp32 master with one
    gradient buffer beside it (engine.ParamStore, as the trunk's).  Names are `prefix` + the name below `bert`'s owner
    ("bert.encoder.layer.0...."): what the model's named_parameters() calls them.  Laid out in reverse execution order --
    layer n-1 first, down to layer 0, then the embeddings -- so that a finished slice can be exchanged while backward
    continues; `sections` = {"layer{i}": (lo, hi), "embeddings": (lo, hi)} in elements.  The weight shadows keep the
    stack's layout ([Wq; Wk; Wv] as one [3d, ld] block, Wo, Wi, Wo2; keys "layer{i}.qkv" / ".ao" / ".fc1" / ".fc2") and are
    all plain images of whole matrices: the fused optimizer kernel writes them, and nothing is left for a second pack."""
    cfg = bert.config
    d, I, nl = cfg.hidden_size, cfg.intermediate_size, cfg.num_hidden_layers
    named, bounds = [], []
    for i in reversed(range(nl)):
        lp = dict(bert.encoder.layer[i].named_parameters())
        bounds.append((f"layer{i}", len(named)))
        named += [(f"{prefix}bert.encoder.layer.{i}.{n}", lp[n]) for n in LAYER_PARAMS]
    if embeddings:
        ep = dict(bert.embeddings.named_parameters())
        bounds.append(("embeddings", len(named)))
        named += [(f"{prefix}bert.embeddings.{n}", ep[n]) for n in EMBED_PARAMS]
    for n, p in named:
        if p.dtype != torch.float32:
            raise RuntimeError(f"text_params='flat': {n} is {p.dtype}; the flat store holds float32 parameters")
    st = ParamStore(named, dtype)
    st.prefix = prefix
    st.sections = {}
    for k, (sname, a) in enumerate(bounds):
        st.sections[sname] = (st.off[named[a][0]], st.off[named[bounds[k + 1][1]][0]] if k + 1 < len(bounds) else st.total)
    ld = pad32(d)
    for i in range(nl):
        P = f"{prefix}bert.encoder.layer.{i}."
        st.add_blank_shadow(f"layer{i}.qkv", 3 * d, ld)
        for w in range(3):
            st.add_shadow(f"layer{i}.qkv#{w}", P + _WEIGHTS[w], d, d, base_key=f"layer{i}.qkv", dst_row0=w * d)
        st.add_shadow(f"layer{i}.ao", P + _WEIGHTS[3], d, d)
        st.add_shadow(f"layer{i}.fc1", P + _WEIGHTS[4], I, d)
        st.add_shadow(f"layer{i}.fc2", P + _WEIGHTS[5], d, I)
    st.finalize_shadows()
    st.set_store_written([f"{prefix}bert.encoder.layer.{i}.{w}" for i in range(nl) for w in _WEIGHTS])
    return st


class _Plan:
    """Activation buffers of one (B, L) shape; kept from forward to backward."""

    def __init__(self, st: "BertLayerStack", B: int, L: int):
        d, I, H, nl, dev = st.d, st.I, st.H, st.n_layers, st.device
        ct = ops.ct_torch(st.dtype)
        R, ld, ldI, dhp = L * B, st.ld, st.ldI, st.dhp
        self.B, self.L, self.R = B, L, R
        # deterministic mode, fixed with the plan: the two dense bias gradients that default mode takes as the LayerNorm
        # backwards' cast_colsum ride on their weight-gradient products (colsum_a), and the LayerNorm backwards refuse
        # a launch that would fall back to float atomics (bpm_ln_bwd_det)
        self.det = config.resolve_deterministic(getattr(st, "deterministic", None))
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
        self.x = [z(R, d) for _ in range(nl + 1)]             # layer inputs; x[nl] is the stack's output
        self.xc = [z(R, ld, dt=ct) for _ in range(nl)]
        self.q = [z(B, H, L, dhp, dt=ct) for _ in range(nl)]
        self.k = [z(B, H, L, dhp, dt=ct) for _ in range(nl)]
        self.v = [z(B, H, L, dhp, dt=ct) for _ in range(nl)]
        self.ctx = [z(R, ld, dt=ct) for _ in range(nl)]
        self.lse = [z(B, H, L) for _ in range(nl)]
        self.y1 = [z(R, d) for _ in range(nl)]
        self.x1 = [z(R, d) for _ in range(nl)]
        self.x1c = [z(R, ld, dt=ct) for _ in range(nl)]
        self.u = [z(R, ldI, dt=ct) for _ in range(nl)]
        self.g = [z(R, ldI, dt=ct) for _ in range(nl)]
        self.y2 = [z(R, d) for _ in range(nl)]
        self.stats = [[z(R) for _ in range(4)] for _ in range(nl)]         # mean1, rstd1, mean2, rstd2
        # backward scratch, shared by the layers
        self.dx = [z(R, d), z(R, d)]                          # gradient of a layer's output / input (ping-pong)
        self.dy2, self.dy1, self.dx1 = z(R, d), z(R, d), z(R, d)
        self.dy2c, self.dy1c = z(R, ld, dt=ct), z(R, ld, dt=ct)
        self.dg = z(R, I)
        self.du = z(R, ldI, dt=ct)
        self.dao = z(B, H, L, dhp, dt=ct)
        self.delta = z(B, H, L)
        self.dqkv = z(R, 3 * ld, dt=ct)
        self.stamp = 0
        self.mask: Optional[torch.Tensor] = None
        self.seed, self.training, self.emb_p = 0, False, 0.0
        # embeddings on the HIP path (embed_buffers): pre-LayerNorm sum, its row statistics, its gradient, scatter workspace
        self.s = self.ds = self.emean = self.erstd = self.ews = None

    def embed_buffers(self, st: "BertLayerStack", type_rows: int) -> None:
        if self.s is None:
            z = lambda *s: torch.zeros(*s, device=st.device, dtype=torch.float32)
            self.s, self.ds, self.emean, self.erstd = z(self.R, st.d), z(self.R, st.d), z(self.R), z(self.R)
            self.ews = z(max(1, ops.bert_embed_scatter_ws_bytes(self.R, st.d, type_rows) // 4))


class BertLayerStack:
    """Host driver of `bert.encoder.layer[*]` (see the module docstring).  Holds no parameters: it reads the HF
    modules' and keeps CT shadows of the six weight matrices of every layer."""

    def __init__(self, bert, precision: Optional[str] = None, store: Optional[ParamStore] = None):
        cfg = bert.config
        check_config(cfg)
        self.bert = bert
        self.precision = precision
        self.deterministic: Optional[bool] = None      # None -> config.deterministic(), read when a plan is built
        # text_params = "flat": the layer parameters are views into this store, which owns the CT shadows (written by the
        # fused optimizer kernel) and the flat gradient buffer the backward launches write into
        self.store = store
        self.grad_ready = None                         # callable(gflat, lo, hi) or None: a finished section (GradSync)
        self.d, self.I, self.H, self.n_layers = cfg.hidden_size, cfg.intermediate_size, cfg.num_attention_heads, cfg.num_hidden_layers
        self.dh = self.d // self.H
        self.dhp = dhp_for(self.dh)
        self.scale = self.dh ** -0.5
        self.ld, self.ldI = pad32(self.d), pad32(self.I)
        self.eps = float(cfg.layer_norm_eps)
        self.p_hidden, self.p_probs = float(cfg.hidden_dropout_prob), float(cfg.attention_probs_dropout_prob)
        self.device: Optional[torch.device] = None
        self.dtype = None
        self._plans: Dict[Tuple[int, int], _Plan] = {}
        self._versions = None

    # -- parameters and their CT shadows -----------------------------------------
    def _prepare(self, device: torch.device) -> None:
        prec = self.precision or config.precision()
        dtype = config.dtype_code(prec)                # bf16x3: the f32 path
        params = getattr(self, "params", None) or layer_parameters(self.bert)
        key = (str(device), dtype, tuple(p.data_ptr() for p in params))      # .to() / .cuda() move the storage
        if getattr(self, "_key", None) == key:
            return
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != device:
                raise RuntimeError("text_encoder='hip': BERT layer parameters must be contiguous float32 tensors on the input's device")
        self._key, self.device, self.dtype = key, device, dtype
        self._plans, self._versions = {}, None
        self.params = params
        if self.store is not None:
            if self.store.dtype != dtype or not self.store.still_flat():
                raise RuntimeError("text_params='flat': the flat text store is stale (another precision, or a parameter was "
                                   "re-pointed); BertEncoder rebuilds it before the forward")
            pre = self.store.prefix
            self._names = [f"{pre}bert.encoder.layer.{i}.{n}" for i in range(self.n_layers) for n in LAYER_PARAMS]
            return
        ct = ops.ct_torch(dtype)
        d, I, ld, ldI = self.d, self.I, self.ld, self.ldI
        # shadows per layer: [Wq; Wk; Wv] as one [3d, ld] block (the data gradient reads it as one K = 3d operand),
        # Wo [d, ld], Wi [I, ld], Wo2 [d, ldI]
        per_layer = 3 * d * ld + d * ld + I * ld + d * ldI
        self.shadow = torch.zeros(per_layer * self.n_layers, device=device, dtype=ct)
        esz = self.shadow.element_size()
        self._soff: List[Dict[str, int]] = []
        descs, blk = [], 0
        for i, layer in enumerate(self.bert.encoder.layer):
            named = dict(layer.named_parameters())
            base = i * per_layer
            offs = {"qkv": base, "ao": base + 3 * d * ld, "fc1": base + 4 * d * ld, "fc2": base + 4 * d * ld + I * ld}
            self._soff.append(offs)
            for name, off, rows, cols in ((_WEIGHTS[0], offs["qkv"], d, d), (_WEIGHTS[1], offs["qkv"] + d * ld, d, d),
                                          (_WEIGHTS[2], offs["qkv"] + 2 * d * ld, d, d), (_WEIGHTS[3], offs["ao"], d, d),
                                          (_WEIGHTS[4], offs["fc1"], I, d), (_WEIGHTS[5], offs["fc2"], d, I)):
                pd = PackDesc()
                pd.src, pd.dst = named[name].data_ptr(), self.shadow.data_ptr() + esz * off
                pd.rows, pd.cols, pd.ld, pd.src_ld, pd.dst_ld, pd.blk0 = rows, cols, pad32(cols), cols, pad32(cols), blk
                pd.colscale = None
                blk += (rows * pad32(cols) + 1023) // 1024
                descs.append(pd)
        self._pack = (ops.device_table(descs), len(descs), blk)

    def _sptr(self, layer: int, key: str, elem_off: int = 0) -> int:
        if self.store is not None:
            return self.store.sptr(f"layer{layer}.{key}", elem_off)
        return self.shadow.data_ptr() + self.shadow.element_size() * (self._soff[layer][key] + elem_off)

    def refresh_shadows(self) -> None:
        """Re-pack the CT weight shadows when a parameter changed.  A change is seen through autograd's version counters:
        an optimizer step, `load_state_dict`, `copy_` and any other in-place op on the parameter move them.  A write
        through `p.data` does NOT (EMA swaps, clamping, some checkpoint loaders): call invalidate_shadows() after one, or
        the products keep reading the old weights.  With a flat store the store keeps the shadows (the same rule; after a
        FusedAdam step they are already current and nothing is launched)."""
        if self.store is not None:
            self.store.refresh_shadows()
            return
        sig = tuple(p._version for p in self.params)
        if sig != self._versions:
            ops.pack_weights(self.dtype, *self._pack)
            self._versions = sig

    def invalidate_shadows(self) -> None:
        """The next forward re-packs the weight shadows whatever the version counters say."""
        self._versions = None
        if self.store is not None:
            self.store.mark_dirty()

    def _plan(self, B: int, L: int) -> _Plan:
        det = config.resolve_deterministic(self.deterministic)
        key = (B, L, "det") if det else (B, L)               # a plan keeps the mode it was built in
        pl = self._plans.get(key)
        if pl is None:
            if len(self._plans) >= 2:                         # activation sets are large: keep the two most recent shapes
                self._plans.pop(next(iter(self._plans)))
            pl = self._plans[key] = _Plan(self, B, L)
        return pl

    def _P(self, layer: int, name: str) -> torch.Tensor:
        return self.params[layer * len(LAYER_PARAMS) + LAYER_PARAMS.index(name)]

    # -- forward ---------------------------------------------------------------------
    def forward(self, emb: Optional[torch.Tensor], mask_u8: torch.Tensor, seed: int, training: bool,
                embed=None) -> Tuple[torch.Tensor, _Plan]:
        """emb fp32 [B, L, d] (the embeddings module's output), mask_u8 uint8 [B, L] -> last hidden state [B, L, d].
        `embed` (with emb None): a callable(plan) that fills the plan's x[0] and xc[0] itself (the HIP embeddings): the
        transposing copy of emb and the first cast launch are then not made."""
        if embed is None:
            B, L, d = emb.shape
        else:
            (B, L), d = mask_u8.shape, self.d
        self._prepare(mask_u8.device if embed is not None else emb.device)
        self.refresh_shadows()
        pl = self._plan(B, L)
        pl.stamp += 1
        pl.mask, pl.seed, pl.training = mask_u8, seed, training
        dt, R, ld, ldI, I, H = self.dtype, pl.R, self.ld, self.ldI, self.I, self.H
        heads = (B, H, L, self.dh, self.dhp)
        ph = self.p_hidden if training else 0.0
        pp = self.p_probs if training else 0.0
        km = ops.attn_kmasks([(mask_u8, L)])
        if embed is None:
            pl.x[0].view(L, B, d).copy_(emb.transpose(0, 1))     # time-major rows
        else:
            embed(pl)
        for i in range(self.n_layers):
            P = lambda n, i=i: self._P(i, n)
            x, xc = pl.x[i], pl.xc[i]
            if i or embed is None:
                ops.rows_cast(dt, [ops.cast_problem(x, d, R, d, dst_ct=xc, ldd=ld)], 0)
            qkv = [ops.gemm_problem(xc, self._sptr(i, "qkv", w * d * ld), out, R, d, d, ld, ld, 0, bias_n=P(f"attention.self.{nm}.bias"),
                                    alpha=self.scale if w == 0 else 1.0, out_kind=OUT_HEADS, heads=heads, flags=F_KPAD)
                   for w, (nm, out) in enumerate((("query", pl.q[i]), ("key", pl.k[i]), ("value", pl.v[i])))]
            ops.gemm_grouped(dt, GEMM_NT, qkv, seed)
            ops.attn_fwd_kmask(dt, [ops.attn_problem(pl.q[i], pl.k[i], pl.v[i], pl.ctx[i], ld, pl.lse[i], B, H, L, L, self.dh, self.dhp,
                                                     0, drop_p=pp, drop_site=bert_site(i, S_PROBS))], km, seed)
            ops.gemm_grouped(dt, GEMM_NT, [ops.gemm_problem(pl.ctx[i], self._sptr(i, "ao"), pl.y1[i], R, d, d, ld, ld, d,
                                                            bias_n=P("attention.output.dense.bias"), resid=x, ldr=d, drop_p=ph,
                                                            drop_site=bert_site(i, S_ATT_OUT), flags=F_KPAD)], seed)
            m1, r1, m2, r2 = pl.stats[i]
            ops.ln_fwd(dt, [ops.ln_problem(pl.y1[i], P("attention.output.LayerNorm.weight"), P("attention.output.LayerNorm.bias"),
                                           m1, r1, R, out=pl.x1[i], ldo=d, out_f32=True)], d, self.eps)
            ops.rows_cast(dt, [ops.cast_problem(pl.x1[i], d, R, d, dst_ct=pl.x1c[i], ldd=ld)], 0)
            ops.gemm_grouped(dt, GEMM_NT, [ops.gemm_problem(pl.x1c[i], self._sptr(i, "fc1"), pl.u[i], R, I, d, ld, ld, ldI,
                                                            bias_n=P("intermediate.dense.bias"), out_kind=OUT_CT, flags=F_KPAD)], seed)
            ops.gelu_fwd(dt, [ops.gelu_problem(pl.u[i], ldI, R, I, u_is_ct=True, g=pl.g[i], ldg=ldI)])
            ops.gemm_grouped(dt, GEMM_NT, [ops.gemm_problem(pl.g[i], self._sptr(i, "fc2"), pl.y2[i], R, d, I, ldI, ldI, d,
                                                            bias_n=P("output.dense.bias"), resid=pl.x1[i], ldr=d, drop_p=ph,
                                                            drop_site=bert_site(i, S_FFN_OUT), flags=F_KPAD)], seed)
            ops.ln_fwd(dt, [ops.ln_problem(pl.y2[i], P("output.LayerNorm.weight"), P("output.LayerNorm.bias"), m2, r2, R,
                                           out=pl.x[i + 1], ldo=d, out_f32=True)], d, self.eps)
        return pl.x[self.n_layers].view(L, B, d).transpose(0, 1).contiguous(), pl

    # -- backward ----------------------------------------------------------------------
    def backward(self, pl: _Plan, dout: torch.Tensor, need_demb: bool, raw: bool = False) -> Tuple[Optional[torch.Tensor], List[torch.Tensor]]:
        """dout fp32 [B, L, d] -> (d(emb) [B, L, d] or None, the gradients of layer_parameters() in order).  Fresh tensors
        every call (autograd may keep them as .grad).  raw: d(emb) is handed back as the plan's own time-major buffer
        [L*B, d] (pl.dx[0] or pl.dx[1]; the other one is free scratch) instead of a batch-major copy."""
        B, L, R = pl.B, pl.L, pl.R
        d, I, H, ld, ldI, dt, seed = self.d, self.I, self.H, self.ld, self.ldI, self.dtype, pl.seed
        heads = (B, H, L, self.dh, self.dhp)
        ph = self.p_hidden if pl.training else 0.0
        pp = self.p_probs if pl.training else 0.0
        km = ops.attn_kmasks([(pl.mask, L)])
        # weight gradients are WRITTEN by their launch; the vectors (biases, LayerNorm affines) are accumulated into: zeroed
        wacc = 0
        if self.store is not None:
            # the store's gradient views, under the trunk's rules: unset gradients -> the weight-gradient launches store
            # and one launch clears everything else; otherwise (an accumulation micro-step) every launch adds
            self._fresh_bwd = self.store.begin_backward(stores=True)
            if not self._fresh_bwd:
                wacc = F_ACCUM
            grads = [self.store.g(n) for n in self._names]
        else:
            wsize = self.n_layers * (4 * d * d + 2 * d * I)
            vsize = self.n_layers * (9 * d + I)
            gw = torch.empty(wsize, device=self.device, dtype=torch.float32)
            gv = torch.zeros(vsize, device=self.device, dtype=torch.float32)
            grads: List[torch.Tensor] = []
            ow = ov = 0
            for p in self.params:
                n = p.numel()
                if p.dim() == 2:
                    grads.append(gw[ow:ow + n].view_as(p))
                    ow += n
                else:
                    grads.append(gv[ov:ov + n].view_as(p))
                    ov += n
        G = lambda i, n: grads[i * len(LAYER_PARAMS) + LAYER_PARAMS.index(n)]
        cur = 0
        pl.dx[cur].view(L, B, d).copy_(dout.transpose(0, 1))
        ln_bwd = lambda probs, *a: ops.ln_bwd(probs, *a, deterministic=pl.det)
        route = (lambda g: (None, g)) if pl.det else (lambda g: (g, None))      # (cast_colsum, colsum_a) of a dense bias gradient
        for i in reversed(range(self.n_layers)):
            P = lambda n, i=i: self._P(i, n)
            dxo, dxi = pl.dx[cur], pl.dx[cur ^ 1]
            m1, r1, m2, r2 = pl.stats[i]
            # output LayerNorm; its cast output is d(output.dense result) = dropmask(dy2) as CT, column sums = the dense bias gradient
            ob_sum, ob_ride = route(G(i, "output.dense.bias"))
            ln_bwd([ops.ln_problem(pl.y2[i], P("output.LayerNorm.weight"), None, m2, r2, R, dy=dxo, ldy=d, dx=pl.dy2,
                                   dgamma=G(i, "output.LayerNorm.weight"), dbeta=G(i, "output.LayerNorm.bias"), cast=pl.dy2c, ldc=ld,
                                   cast_colsum=ob_sum, drop_p=ph, drop_site=bert_site(i, S_FFN_OUT))], d, dt, seed)
            ops.gemm_grouped(dt, GEMM_TN, [ops.gemm_problem(pl.dy2c, pl.g[i], G(i, "output.dense.weight"), d, I, R, ld, ldI, I,
                                                            colsum_a=ob_ride, flags=F_KPAD | wacc)], seed)
            ops.gemm_grouped(dt, GEMM_NN, [ops.gemm_problem(pl.dy2c, self._sptr(i, "fc2"), pl.dg, R, I, d, ld, ldI, I, out_kind=OUT_F32,
                                                            flags=F_KPAD)], seed)
            ops.gelu_bwd(dt, [ops.gelu_problem(pl.u[i], ldI, R, I, u_is_ct=True, dg=pl.dg, lddg=I, du=pl.du, lddu=ldI)])
            ops.gemm_grouped(dt, GEMM_TN, [ops.gemm_problem(pl.du, pl.x1c[i], G(i, "intermediate.dense.weight"), I, d, R, ldI, ld, d,
                                                            colsum_a=G(i, "intermediate.dense.bias"), flags=F_KPAD | wacc)], seed)
            # d(x1) = du Wi + dy2 (the residual branch rides in the epilogue)
            ops.gemm_grouped(dt, GEMM_NN, [ops.gemm_problem(pl.du, self._sptr(i, "fc1"), pl.dx1, R, d, I, ldI, ld, d, resid=pl.dy2, ldr=d,
                                                            flags=F_KPAD)], seed)
            ab_sum, ab_ride = route(G(i, "attention.output.dense.bias"))
            ln_bwd([ops.ln_problem(pl.y1[i], P("attention.output.LayerNorm.weight"), None, m1, r1, R, dy=pl.dx1, ldy=d, dx=pl.dy1,
                                   dgamma=G(i, "attention.output.LayerNorm.weight"), dbeta=G(i, "attention.output.LayerNorm.bias"),
                                   cast=pl.dy1c, ldc=ld, cast_colsum=ab_sum, drop_p=ph,
                                   drop_site=bert_site(i, S_ATT_OUT))], d, dt, seed)
            ops.gemm_grouped(dt, GEMM_TN, [ops.gemm_problem(pl.dy1c, pl.ctx[i], G(i, "attention.output.dense.weight"), d, d, R, ld, ld, d,
                                                            colsum_a=ab_ride, flags=F_KPAD | wacc)], seed)
            ops.gemm_grouped(dt, GEMM_NN, [ops.gemm_problem(pl.dy1c, self._sptr(i, "ao"), pl.dao, R, d, d, ld, ld, 0, out_kind=OUT_HEADS,
                                                            heads=heads, flags=F_KPAD)], seed)
            dq, dk, dv = pl.dqkv[:, :ld], pl.dqkv[:, ld:2 * ld], pl.dqkv[:, 2 * ld:]
            ap = [ops.attn_problem(pl.q[i], pl.k[i], pl.v[i], pl.ctx[i], ld, pl.lse[i], B, H, L, L, self.dh, self.dhp, 0, dO=pl.dao,
                                   delta=pl.delta, dQ=dq, lddq=3 * ld, dK=dk, lddk=3 * ld, dV=dv, lddv=3 * ld, dq_scale=self.scale,
                                   drop_p=pp, drop_site=bert_site(i, S_PROBS))]
            ops.attn_bwd_dq_kmask(dt, ap, km, seed)
            ops.attn_bwd_dkv_kmask(dt, ap, km, seed)
            ops.gemm_grouped(dt, GEMM_TN, [ops.gemm_problem(src, pl.xc[i], G(i, f"attention.self.{nm}.weight"), d, d, R, 3 * ld, ld, d,
                                                            colsum_a=G(i, f"attention.self.{nm}.bias"), flags=F_KPAD | wacc)
                                           for nm, src in (("query", dq), ("key", dk), ("value", dv))], seed)
            # d(x) = dq Wq + dk Wk + dv Wv + dy1
            # (one K = 3d product: check_config admits only d % 32 == 0, so ld == d and [dq | dk | dv] has no pad columns)
            ops.gemm_grouped(dt, GEMM_NN, [ops.gemm_problem(pl.dqkv, self._sptr(i, "qkv"), dxi, R, d, 3 * d, 3 * ld, ld, d,
                                                            resid=pl.dy1, ldr=d, flags=F_KPAD)], seed)
            cur ^= 1
            if self.store is not None and self.grad_ready is not None:
                self.grad_ready(self.store.gflat, *self.store.sections[f"layer{i}"])
        if raw:
            return (pl.dx[cur] if need_demb else None), grads
        demb = pl.dx[cur].view(L, B, d).transpose(0, 1).contiguous() if need_demb else None
        return demb, grads


    def finish_backward(self) -> None:
        """Flat store: `.grad` of every stored parameter becomes its view of the store's gradient buffer (after the last
        launch that writes it: the embeddings' when they are HIP kernels)."""
        if self.store is not None:
            self.store.end_backward()


class _StackFn(torch.autograd.Function):
    """The BERT layer stack as one autograd node: (embedding output, byte mask, layer parameters) -> last hidden state."""

    @staticmethod
    def forward(ctx, emb, mask_u8, stack, seed, training, *params):
        out, plan = stack.forward(emb.detach().contiguous().float(), mask_u8, seed, training)
        ctx.stack, ctx.plan, ctx.stamp = stack, plan, plan.stamp
        ctx.need_emb = emb.requires_grad
        ctx.need_params = [p.requires_grad for p in params]
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.stamp != ctx.plan.stamp:
            raise RuntimeError("text encoder (HIP path): backward() of a forward pass that a later forward pass of the same shape "
                               "has overwritten; run forward -> backward one step at a time")
        demb, grads = ctx.stack.backward(ctx.plan, dout.contiguous().float(), ctx.need_emb)
        if ctx.stack.store is not None:                    # the launches wrote the store's gradient buffer: nothing to hand back
            ctx.stack.finish_backward()
            return (demb, None, None, None, None) + (None,) * len(grads)
        return (demb, None, None, None, None) + tuple(g if need else None for g, need in zip(grads, ctx.need_params))


def run_layers(stack: BertLayerStack, emb: torch.Tensor, mask: Optional[torch.Tensor], seed: int, training: bool) -> torch.Tensor:
    """emb [B, L, d] (output of bert.embeddings), mask [B, L] (HF attention_mask: non-zero = a real token; None = all) ->
    last hidden state [B, L, d] through the HIP layer stack."""
    if not emb.is_cuda:
        raise RuntimeError("text encoder: the HIP layer stack needs CUDA (HIP) tensors; there is no CPU path")
    B, L = emb.shape[0], emb.shape[1]
    if mask is None:
        mask_u8 = torch.ones(B, L, device=emb.device, dtype=torch.uint8)
    else:
        if mask.shape != (B, L):
            raise ValueError(f"text encoder: attention mask of shape {tuple(mask.shape)} for inputs of shape {(B, L)}")
        mask_u8 = (mask.to(emb.device) != 0).to(torch.uint8).contiguous()        # on the device: no length reaches the host
    stack._prepare(emb.device)
    return _StackFn.apply(emb, mask_u8, stack, seed, training, *stack.params)


# ---------------------------------------------------------------------------------------------------------------------
# embeddings on the HIP path (args.text_embeddings = "hip")
# ---------------------------------------------------------------------------------------------------------------------
EMBED_PARAMS = ("word_embeddings.weight", "position_embeddings.weight", "token_type_embeddings.weight", "LayerNorm.weight",
                "LayerNorm.bias")


def check_embed_config(cfg) -> None:
    """What the HIP embeddings implement beyond check_config()."""
    if cfg.hidden_size > MAX_EMBED_HIDDEN:
        raise ValueError(f"text_embeddings='hip': hidden_size {cfg.hidden_size} > {MAX_EMBED_HIDDEN} is beyond the reach of the "
                         "16-byte row kernels")


def check_positions(L: int, cfg) -> None:
    if L > cfg.max_position_embeddings:
        raise ValueError(f"text encoder: {L} tokens per sample, but the model has max_position_embeddings = "
                         f"{cfg.max_position_embeddings}")


def embed_parameters(bert) -> List[torch.nn.Parameter]:
    named = dict(bert.embeddings.named_parameters())
    return [named[n] for n in EMBED_PARAMS]


class BertEmbeddingsHip:
    """Host driver of `bert.embeddings` on the HIP path.  Holds no parameters: it reads the HF module's tables and
    LayerNorm affine where they lie.  `bad` is the int32 device counter of ids outside their table (cumulative)."""

    def __init__(self, bert, bad: torch.Tensor, store: Optional[ParamStore] = None):
        check_embed_config(bert.config)
        self.bert, self.bad = bert, bad
        self.store = store                                 # text_params = "flat": the five parameters live in this store
        self._scratch: Optional[torch.Tensor] = None      # table gradients of an accumulation micro-step (allocated once)
        self.eps = float(bert.config.layer_norm_eps)
        self.padding_idx = bert.embeddings.word_embeddings.padding_idx

    def parameters(self) -> List[torch.nn.Parameter]:
        params = embed_parameters(self.bert)
        for p in params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != self.bad.device:
                raise RuntimeError("text_embeddings='hip': BERT embedding parameters must be contiguous float32 tensors on the input's device")
        return params

    def drop_p(self, training: bool) -> float:
        return float(self.bert.embeddings.dropout.p) if training else 0.0

    def forward(self, st: BertLayerStack, pl: _Plan, ids: torch.Tensor, seg: Optional[torch.Tensor], seed: int, training: bool) -> None:
        word, pos, typ, gamma, beta = self.parameters()
        pl.embed_buffers(st, typ.shape[0])
        pl.emb_p = self.drop_p(training)
        prob = ops.bert_embed_problem(ids, seg, word, pos, typ, gamma, beta, x=pl.x[0], xc=pl.xc[0], ldc=st.ld, s=pl.s, mean=pl.emean,
                                      rstd=pl.erstd, bad=self.bad, drop_p=pl.emb_p, drop_site=bert_site(0, S_EMBED))
        ops.bert_embed_fwd(st.dtype, prob, st.d, self.eps, seed)

    def backward(self, st: BertLayerStack, pl: _Plan, dy: torch.Tensor, ids: torch.Tensor, seg: Optional[torch.Tensor],
                 need: List[bool]) -> List[Optional[torch.Tensor]]:
        """dy: the stack's time-major d(x[0]) buffer (pl.dx[0] or pl.dx[1]) -> gradients of EMBED_PARAMS (None where not
        needed).  Launches nothing when nothing is needed."""
        if not any(need):
            return [None] * 5
        word, pos, typ, gamma, beta = self.parameters()
        d, R, dev = st.d, pl.R, st.device
        if pl.emb_p > 0.0:                                # regenerate the forward's mask into the free ping-pong buffer
            g = pl.dx[1] if dy is pl.dx[0] else pl.dx[0]
            ops.rows_cast(st.dtype, [ops.cast_problem(dy, d, R, d, dst_f32=g, ldf=d, drop_p=pl.emb_p, drop_site=bert_site(0, S_EMBED))],
                          pl.seed)
            dy = g
        affine = need[3] or need[4]
        if self.store is not None:
            return self._backward_flat(st, pl, dy, ids, seg, need, (word, pos, typ, gamma, beta))
        gv = torch.zeros(2, d, device=dev, dtype=torch.float32) if affine else None
        ops.ln_bwd([ops.ln_problem(pl.s, gamma, None, pl.emean, pl.erstd, R, dy=dy, ldy=d, dx=pl.ds,
                                   dgamma=gv[0] if affine else None, dbeta=gv[1] if affine else None)], d, st.dtype, pl.seed,
                   deterministic=pl.det)
        out: List[Optional[torch.Tensor]] = [None, None, None, gv[0] if need[3] else None, gv[1] if need[4] else None]
        if any(need[:3]):
            kw = {}
            if need[0]:
                sid, perm = torch.sort(ids.view(-1), stable=True)         # integer plumbing on the device, no sync
                out[0] = torch.zeros_like(word)
                kw.update(sorted_ids=sid, perm=perm, dword=out[0], padding_idx=self.padding_idx)
            if need[1]:
                out[1] = torch.zeros_like(pos)
                kw.update(dpos=out[1])
            if need[2]:
                out[2] = torch.zeros_like(typ)
                kw.update(dtype_=out[2])
            ops.bert_embed_scatter(ops.bert_scatter_problem(pl.ds, pl.B, pl.L, pl.ews, seg=seg, **kw), d)
        return out


    def _backward_flat(self, st: BertLayerStack, pl: _Plan, dy, ids, seg, need, params) -> List[None]:
        """The same launches writing the store's gradient views.  The LayerNorm affine gradients are accumulated into
        (cleared with the other vectors when the gradients were unset).  bpm_bert_embed_scatter STORES its rows: on a fresh
        step it writes the cleared table slices themselves; on an accumulation micro-step it writes a scratch copy of the
        three tables' slice (kept, cleared here), which one bpm_add_n then adds in -- one fp32 add per element, the bits of
        autograd's `+=`."""
        store, d = self.store, st.d
        names = [f"{store.prefix}bert.embeddings.{n}" for n in EMBED_PARAMS]
        g = [store.g(n) for n in names]
        ops.ln_bwd([ops.ln_problem(pl.s, params[3], None, pl.emean, pl.erstd, pl.R, dy=dy, ldy=d, dx=pl.ds,
                                   dgamma=g[3] if need[3] or need[4] else None, dbeta=g[4] if need[3] or need[4] else None)],
                   d, st.dtype, pl.seed, deterministic=pl.det)
        if any(need[:3]):
            lo = store.off[names[0]]
            hi = store.off[names[2]] + (params[2].numel() + store.ALIGN - 1) // store.ALIGN * store.ALIGN
            if st._fresh_bwd:
                dst = g[:3]
            else:
                if self._scratch is None or self._scratch.numel() != hi - lo:
                    self._scratch = torch.zeros(hi - lo, device=store.device, dtype=torch.float32)
                else:
                    self._scratch.zero_()
                dst = [self._scratch[store.off[n] - lo: store.off[n] - lo + p.numel()].view(p.shape) for n, p in zip(names, params[:3])]
            kw = {}
            if need[0]:
                sid, perm = torch.sort(ids.view(-1), stable=True)         # integer plumbing on the device, no sync
                kw.update(sorted_ids=sid, perm=perm, dword=dst[0], padding_idx=self.padding_idx)
            if need[1]:
                kw.update(dpos=dst[1])
            if need[2]:
                kw.update(dtype_=dst[2])
            ops.bert_embed_scatter(ops.bert_scatter_problem(pl.ds, pl.B, pl.L, pl.ews, seg=seg, **kw), d)
            if not st._fresh_bwd:
                ops.add_n([ops.addn_problem(store.gflat[lo:hi], [store.gflat[lo:hi], self._scratch])])
        return [None] * 5


class _EncoderFn(torch.autograd.Function):
    """Embeddings + layer stack as ONE autograd node: (ids, type ids, byte mask, the five embedding parameters, the layer
    parameters) -> last hidden state."""

    @staticmethod
    def forward(ctx, ids, seg, mask_u8, stack, embd, seed, training, *params):
        out, plan = stack.forward(None, mask_u8, seed, training, embed=lambda pl: embd.forward(stack, pl, ids, seg, seed, training))
        ctx.stack, ctx.embd, ctx.plan, ctx.stamp, ctx.ids, ctx.seg = stack, embd, plan, plan.stamp, ids, seg
        ctx.need = [p.requires_grad for p in params]
        return out

    @staticmethod
    def backward(ctx, dout):
        if ctx.stamp != ctx.plan.stamp:
            raise RuntimeError("text encoder (HIP path): backward() of a forward pass that a later forward pass of the same shape "
                               "has overwritten; run forward -> backward one step at a time")
        need_e, need_l = ctx.need[:5], ctx.need[5:]
        dx, grads = ctx.stack.backward(ctx.plan, dout.contiguous().float(), any(need_e), raw=True)
        egrads = ctx.embd.backward(ctx.stack, ctx.plan, dx, ctx.ids, ctx.seg, need_e)
        store = ctx.stack.store
        if store is not None:
            if ctx.stack.grad_ready is not None:
                ctx.stack.grad_ready(store.gflat, *store.sections["embeddings"])
            ctx.stack.finish_backward()
            return (None,) * (7 + len(ctx.need))
        return (None,) * 7 + tuple(egrads) + tuple(g if n else None for g, n in zip(grads, need_l))


def run_encoder(stack: BertLayerStack, embd: BertEmbeddingsHip, ids: torch.Tensor, mask: Optional[torch.Tensor],
                seg: Optional[torch.Tensor], seed: int, training: bool) -> torch.Tensor:
    """ids [B, L] (token ids), mask [B, L] (HF attention_mask; None = all), seg [B, L] (token type ids; None = zeros) ->
    last hidden state [B, L, d]: HIP embeddings and HIP layer stack behind one autograd node."""
    if ids.dim() != 2:
        raise ValueError(f"text encoder: token ids of shape {tuple(ids.shape)}, expected [B, L]")
    B, L = ids.shape
    check_positions(L, stack.bert.config)                 # from the shapes, on the host, before the device check
    if not ids.is_cuda:
        raise RuntimeError("text encoder: the HIP layer stack needs CUDA (HIP) tensors; there is no CPU path")
    dev = ids.device
    if seg is not None and seg.shape != (B, L):
        raise ValueError(f"text encoder: token type ids of shape {tuple(seg.shape)} for inputs of shape {(B, L)}")
    if mask is None:
        mask_u8 = torch.ones(B, L, device=dev, dtype=torch.uint8)
    else:
        if mask.shape != (B, L):
            raise ValueError(f"text encoder: attention mask of shape {tuple(mask.shape)} for inputs of shape {(B, L)}")
        mask_u8 = (mask.to(dev) != 0).to(torch.uint8).contiguous()
    ids = ids.long().contiguous()                         # HF passes int64: no launch then
    seg = seg.to(dev).long().contiguous() if seg is not None else None
    stack._prepare(dev)
    return _EncoderFn.apply(ids, seg, mask_u8, stack, embd, seed, training, *embd.parameters(), *stack.params)
