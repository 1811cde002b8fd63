"""BPMulT model graphs on the MI355X engine.

`MultiprojectionMMTransformer3DGMUClf` (3-modal, reference mmtr.py:587-866) and
`MultiprojectionMMTransformerGMUClf` (4-modal, mmtr.py:277-583) keep the
reference's constructor (`args`), forward signature and state_dict names.  The
hot path -- temporal 1x1 projections, the twelve crossmodal / biprojection
encoders, the dense Fusion-GMU layers, the time-axis maps, and the [B,d] tail
(level 1->3 residual + token pick, final n-way GMU, residual head) -- runs as
grouped HIP launches orchestrated by `_Trunk` behind ONE autograd node
(`_ModelFn`): features in, (logits, gates) out.  The front-ends upstream of
the path: the text encoder is an ordinary PyTorch-ROCm module (HF BERT from a
local directory); the AudioEncoder convolution stack and the poster projection
run on this library's GEMM and row kernels (frontend.py).

Deliberate departures from the reference's *behaviour as shipped* (all listed
in SURVEY.md section 0): the 3-modal final GMU takes three inputs (the
reference's 4-argument call to a 5-argument constructor cannot be built);
zero-padding is device agnostic; `--hybrid` is not supported (broken upstream).
"""
from __future__ import annotations

import os
from typing import Dict, List, Optional, Sequence, Tuple

import torch
from torch import nn

from .. import config, ops
from .._lib import (BPM_F32, F_ACCUM, GEMM_NN, GEMM_NT, GEMM_TN, AddnProblem, CastProblem, GemmProblem, GmuProblem, TailDesc,
                    TailGrads)
from ..engine import SITE_TEXT, EncoderDesc, EncoderGroupPlan, GroupCfg, ParamStore, register_encoder_shadows
from ..graphs import _RETIRED_GRAPHS, GraphCache  # noqa: F401  (_RETIRED_GRAPHS: read through this module too)
from ..ops import pad32
from .encoder import TransformerEncoder

# encoder name -> (query modality, key/value source, attention-dropout key = last letter of the reference tag)
LEVEL1 = {"trans_v_with_a": ("v", "a", "a"), "trans_a_with_v": ("a", "v", "v"), "trans_v_with_l": ("v", "l", "l"),
          "trans_l_with_v": ("l", "v", "v"), "trans_a_with_l": ("a", "l", "l"), "trans_l_with_a": ("l", "a", "a")}
# level 2: key/value source is a level-1 OUTPUT (mmtr.py:790-791, 812-813, 834-835)
LEVEL2 = {"trans_l_with_v2a": ("l", "trans_a_with_v", "a"), "trans_l_with_a2v": ("l", "trans_v_with_a", "v"),
          "trans_a_with_v2l": ("a", "trans_l_with_v", "l"), "trans_a_with_l2v": ("a", "trans_v_with_l", "v"),
          "trans_v_with_a2l": ("v", "trans_l_with_a", "l"), "trans_v_with_l2a": ("v", "trans_a_with_l", "a")}
# fusion per target modality: (lvl2_a, lvl1_a, lvl2_b, lvl1_b); the middle GMU takes (lvl1_a, lvl1_b)
# (argument order of mmtr.py:796-803, 818-825, 840-847)
FUSE = {"l": ("trans_l_with_a2v", "trans_v_with_a", "trans_l_with_v2a", "trans_a_with_v"),
        "a": ("trans_a_with_v2l", "trans_l_with_v", "trans_a_with_l2v", "trans_v_with_l"),
        "v": ("trans_v_with_a2l", "trans_l_with_a", "trans_v_with_l2a", "trans_a_with_l")}
# 4-modal: level-1 outputs whose length differs from the target's go through a time-axis Linear (mmtr.py:507-508,530,553)
TIME_MAP = {"l": {"trans_v_with_a": "transfm_v2l", "trans_a_with_v": "transfm_a2l"},
            "a": {"trans_l_with_v": "transfm_l2a"},
            "v": {"trans_l_with_a": "transfm_l2v"}}
ENC_ORDER = list(LEVEL1) + list(LEVEL2)


class GatedMultimodalLayerFeatures(nn.Module):
    """Fusion-GMU parameters (mmtr.py:179-188); evaluated by the trunk."""

    def __init__(self, size_in1, size_in2, size_out):
        super().__init__()
        self.hidden1 = nn.Linear(size_in1, size_out, bias=False)
        self.hidden2 = nn.Linear(size_in2, size_out, bias=False)
        self.x_gate = nn.Linear(size_in1 + size_in2, size_out, bias=False)


class TextShiftingLayer(nn.Module):
    """Parameters of the final n-way gated fusion on [B,d] rows (TextShifting3Layer / TextShifting4Layer,
    mmtr.py:197-247): sum_i sigmoid(G_i [x_1|..|x_n]) * tanh(W_i x_i).  Evaluated by the tail kernels
    (csrc/tail.hip, bpm_tail_fwd / bpm_tail_bwd); no PyTorch forward."""

    def __init__(self, sizes_in: Sequence[int], size_out: int):
        super().__init__()
        tot = sum(sizes_in)
        for i, s in enumerate(sizes_in, 1):
            setattr(self, f"hidden{i}", nn.Linear(s, size_out, bias=False))
            setattr(self, f"x{i}_gate", nn.Linear(tot, size_out, bias=False))
        self.n = len(sizes_in)


class AudioEncoder(nn.Module):
    """Front-end of the 4-modal model (mmtr.py:93-108): Conv1d(96,96,128,stride 2) x 2 + AdaptiveAvgPool1d(200).  The
    modules below only hold the parameters under the reference's names; `encode` runs the stack on the HIP path
    (frontend.py: the convolutions as implicit products of the grouped MFMA GEMM over the channels-last signal + pooling kernels) and returns [B, 200, 96], i.e. the reference's
    `audio_enc(audio).transpose(1, 2)`."""

    def __init__(self, args=None):
        super().__init__()
        self.conv_layers = nn.ModuleList([nn.Conv1d(96, 96, 128, stride=2), nn.Conv1d(96, 96, 128, stride=2),
                                          nn.AdaptiveAvgPool1d(200)])

    def encode(self, x, precision: str):
        from ..frontend import audio_encoder_forward
        pool = self.conv_layers[2].output_size
        pool = pool[0] if isinstance(pool, (tuple, list)) else pool
        return audio_encoder_forward(x, (self.conv_layers[0], self.conv_layers[1]), int(pool), precision)


TEXT_ENCODERS = ("torch", "hip")
TEXT_EMBEDDINGS = ("torch", "hip")
TEXT_PARAMS = ("torch", "flat")


def step_seed(step: int) -> int:
    """Dropout seed of forward pass number `step`: (process seed, data-parallel rank, step).  Ranks that seed alike must
    still draw independent masks on their shards, as the reference's DataParallel replicas do.  The one formula of the
    trunk (_BPMulTBase._next_seed) and of the HIP text encoder (BertEncoder._next_seed)."""
    rank = torch.distributed.get_rank() if (torch.distributed.is_available() and torch.distributed.is_initialized()) else 0
    return (torch.initial_seed() * 1000003 + rank * 0x9E3779B97F4A7C15 + int(step)) & 0x7FFFFFFFFFFFFFFF   # 63 bits: bit 63 marks an indirect seed


class BertEncoder(nn.Module):
    """Text encoder plug point (mmtr.py:144-158).  `args.bert_model` may be a local
    HF directory; with `args.text_features=True` (synthetic benchmarks, parity
    tests) the `txt` argument already holds [B,L,orig_d_l] features.

    `args.text_encoder`: "torch" (the default: HF `BertModel` as it is) or "hip": `self.bert` is the same HF module (same
    parameters, same state_dict keys), its embeddings run on torch (by default), and its `encoder.layer[*]` stack runs on the HIP
    path behind one autograd node (models/bert.py); the pooler, whose output the reference discards, is not evaluated.

    `args.text_embeddings`: "torch" (the default) or "hip" (needs text_encoder = "hip" and hidden_size <= 1024): the
    embeddings (three gathers, LayerNorm, dropout from the library's keyed hash) are HIP kernels too, and ids -> last
    hidden state is ONE autograd node with bit-reproducible embedding gradients.  `bad_token_ids`: an int32 device counter
    of token / type ids outside their table met so far (each contributes a zero row; reading it is the caller's sync).

    `args.text_params`: "torch" (the default: the BERT parameters are PyTorch's, "tail" parameters of FusedAdam) or "flat"
    (needs text_encoder = "hip"): the parameters whose gradients the HIP path produces live in a flat store of their own
    (`flat_store()`), the backward writes their gradients there and FusedAdam steps them in the trunk's launch."""

    def __init__(self, args):
        super().__init__()
        self.features_in = bool(getattr(args, "text_features", False))
        self.text_encoder = getattr(args, "text_encoder", "torch")
        if self.text_encoder not in TEXT_ENCODERS:
            raise ValueError(f"text_encoder must be one of {TEXT_ENCODERS}, got {self.text_encoder!r}")
        self.text_embeddings = getattr(args, "text_embeddings", "torch")
        if self.text_embeddings not in TEXT_EMBEDDINGS:
            raise ValueError(f"text_embeddings must be one of {TEXT_EMBEDDINGS}, got {self.text_embeddings!r}")
        if self.text_embeddings == "hip" and self.text_encoder != "hip":
            raise ValueError("text_embeddings='hip' needs text_encoder='hip' (the embeddings feed the HIP layer stack's buffers)")
        self.text_params = getattr(args, "text_params", "torch")
        if self.text_params not in TEXT_PARAMS:
            raise ValueError(f"text_params must be one of {TEXT_PARAMS}, got {self.text_params!r}")
        if self.text_params == "flat" and self.text_encoder != "hip":
            raise ValueError("text_params='flat' needs text_encoder='hip' (the flat store holds the parameters whose gradients "
                             "the HIP layer stack writes)")
        self.precision: Optional[str] = getattr(args, "precision", None)
        flag = getattr(args, "deterministic", None)             # None: config.deterministic(), read when the stack builds a plan
        self.deterministic: Optional[bool] = None if flag is None else bool(flag)
        self.bert = None
        self.store_prefix = ""          # this module's name in the model ("enc."): the flat store uses the model's parameter names
        self._text_store = None
        self._grad_ready = None         # set by the model: callable(gflat, lo, hi) for a finished section of the text store
        self._stack = None
        self._embd = None
        self.bad_token_ids: Optional[torch.Tensor] = None       # device counter, created by the first HIP-embeddings forward
        self.dropout_step = 0           # host-side step counter of the HIP stack's dropout stream (the model sets it per step)
        if not self.features_in:
            from transformers import BertModel  # local directory only: there is no network
            self.bert = BertModel.from_pretrained(args.bert_model)
            if self.text_encoder == "hip":
                from .bert import check_config
                check_config(self.bert.config)
                if self.text_embeddings == "hip":
                    from .bert import check_embed_config
                    check_embed_config(self.bert.config)

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._stack = None              # shadows and activation buffers live on the old device
        self._embd = None
        self._text_store = None
        self.bad_token_ids = None
        return r

    def flat_store(self):
        """`text_params = "flat"`: the engine.ParamStore of the text parameters whose gradients the HIP path produces --
        the 16 parameters of every `bert.encoder.layer[i]` and, with `text_embeddings = "hip"`, the five embedding
        parameters; the pooler (and the embeddings on torch) stay PyTorch's.  The module tree, named_parameters() and the
        state_dict keys are unchanged: the parameters become views into the store's master.  Built at the first use and
        again after anything re-pointed a parameter (.to() / .cuda(), `p.data = ...`) or changed the precision; None with
        `text_params = "torch"` or text features.  The parameters must be on the GPU."""
        if self.text_params != "flat" or self.bert is None:
            return None
        dt = config.dtype_code(self.precision or config.precision())
        st = self._text_store
        if st is None or st.dtype != dt or st.prefix != self.store_prefix or not st.still_flat():
            from .bert import build_text_store
            self._text_store = st = build_text_store(self.bert, dt, self.text_embeddings == "hip", self.store_prefix)
            self._stack = self._embd = None
        return st

    def _next_seed(self) -> int:
        self.dropout_step += 1
        return step_seed(self.dropout_step)

    def invalidate_shadows(self) -> None:
        """Call after writing BERT layer weights in a way autograd's version counters do not see (through `p.data`: EMA
        swaps, clamping, some checkpoint loaders): the HIP stack re-packs its CT weight shadows on the next forward.
        Optimizer steps, `load_state_dict`, `copy_` and other in-place ops on the parameters are noticed without it."""
        if self._stack is not None:
            self._stack.invalidate_shadows()
        if self._text_store is not None:
            self._text_store.mark_dirty()

    def forward(self, txt, mask, segment):
        if self.features_in:
            return txt
        if self.text_encoder == "hip":
            from .bert import BertEmbeddingsHip, BertLayerStack, check_positions, run_encoder, run_layers
            if self.text_embeddings == "hip":
                check_positions(txt.shape[-1], self.bert.config)
                if not txt.is_cuda:
                    raise RuntimeError("text encoder: the HIP layer stack needs CUDA (HIP) tensors; there is no CPU path")
            else:
                emb = self.bert.embeddings(input_ids=txt, token_type_ids=segment)
            store = self.flat_store()       # (drops a stack built over an older store)
            if self._stack is None:
                self._stack = BertLayerStack(self.bert, self.precision, store=store)
            self._stack.precision = self.precision
            self._stack.deterministic = self.deterministic
            self._stack.grad_ready = self._grad_ready
            if self.text_embeddings == "hip":
                if self._embd is None:
                    self.bad_token_ids = torch.zeros(1, device=txt.device, dtype=torch.int32)
                    self._embd = BertEmbeddingsHip(self.bert, self.bad_token_ids, store=store)
                return run_encoder(self._stack, self._embd, txt, mask, segment, self._next_seed(), self.training)
            return run_layers(self._stack, emb, mask, self._next_seed(), self.training)
        return self.bert(input_ids=txt, token_type_ids=segment, attention_mask=mask, return_dict=False)[0]


# ----------------------------------------------------------------------------
class _Trunk(GraphCache):
    """Device buffers + launch tables of the hot path for one batch size; its captured graphs (GraphCache)."""

    def __init__(self, model: "_BPMulTBase", B: int):
        self.m, self.B = model, B
        st = model._store
        self.st, self.dtype = st, st.dtype
        d = model.d
        self.d, self.ld = d, pad32(d)
        dev = st.device
        ct = ops.ct_torch(self.dtype)
        z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
        self.N = {"l": model.num_vectors_l, "a": model.num_vectors_a, "v": model.num_vectors_v}
        self.px = {k: z(n, B, d) for k, n in self.N.items()}            # projected, zero-padded inputs [N,B,d]
        self.dpx = {k: z(n, B, d) for k, n in self.N.items()}
        cfg1 = GroupCfg(d, model.num_heads, model.layers, model.relu_dropout, model.res_dropout, model.embed_dropout,
                        model.attn_mask, False)
        cfg2 = GroupCfg(d, model.num_heads, model.layers, model.relu_dropout, model.res_dropout, model.embed_dropout,
                        model.attn_mask, model.four_modal)
        adrop = {"l": model.attn_dropout, "a": model.attn_dropout_a, "v": model.attn_dropout_v}
        e1 = [EncoderDesc(n + ".", ENC_ORDER.index(n), self.N[q], self.N[kv], adrop[key]) for n, (q, kv, key) in LEVEL1.items()]
        # Exact dead-row elimination (verified on the reference): in a crossmodal encoder a query row
        # never sees another query row (keys / values come from the other source in every layer), the Fusion-GMU and
        # the level 1 -> 2 / 1 -> 3 residuals are position-wise, and the head consumes only rows 0 and N-1
        # (mmtr.py:522,545,568 / 808,830,852).  3-modal model: the level-2 encoders and the GMUs only need those two
        # query rows.  4-modal model: the level-2 encoders are biprojection encoders whose causal self-attention lets a
        # row see the earlier rows, so only their LAST layer shrinks (its self-attention queries, cross attention, FFN
        # and the final LayerNorm: EncoderDesc.tail_rows); the GMUs and the OUTPUTS of the time-axis maps (two rows of
        # transfm_*, mmtr.py:507-508,530,553) follow.  Level 1 stays dense (it is level 2's key / value source).
        self.prune = bool(getattr(model, "prune_unused_rows", False)) and min(self.N.values()) >= 2
        self.Ng = {k: (2 if self.prune else n) for k, n in self.N.items()}            # rows of level-2 outputs / GMU tensors
        if self.prune:
            self.idx = {k: torch.tensor([0, n - 1], device=dev) for k, n in self.N.items()}
        if self.prune and model.four_modal:
            e2 = [EncoderDesc(n + ".", ENC_ORDER.index(n), self.N[q], self.N[LEVEL1[src][0]], adrop[key], tail_rows=True)
                  for n, (q, src, key) in LEVEL2.items()]
        elif self.prune:
            self.pxg = {k: z(2, B, d) for k in self.N}
            e2 = [EncoderDesc(n + ".", ENC_ORDER.index(n), 2, self.N[LEVEL1[src][0]], adrop[key], q_pos0=0,
                              q_stride=self.N[q] - 1, T_full=self.N[q]) for n, (q, src, key) in LEVEL2.items()]
        else:
            e2 = [EncoderDesc(n + ".", ENC_ORDER.index(n), self.N[q], self.N[LEVEL1[src][0]], adrop[key])
                  for n, (q, src, key) in LEVEL2.items()]
        # bf16x3 mode: the split images of this trunk's activations live and go with it (the weight shadows' with the store)
        self.x3 = ops.X3Cache(dev, weights=st.x3_cache) if st.x3 else None
        self.det = config.resolve_deterministic(getattr(model, "deterministic", None))       # read once, with the tables
        self.plan1 = EncoderGroupPlan(st, cfg1, e1, B, x3=self.x3, deterministic=self.det)
        self.plan2 = EncoderGroupPlan(st, cfg2, e2, B, x3=self.x3, deterministic=self.det)
        self.out1 = {n: b["out"] for n, b in zip(LEVEL1, self.plan1.buf)}
        self.out2 = {n: b["out"] for n, b in zip(LEVEL2, self.plan2.buf)}
        self.d1buf = {n: z(self.N[q], B, d) for n, (q, _, _) in LEVEL1.items()}   # d(level-1 outputs)
        if self.prune:                      # rows 0 and N-1 of the level-1 outputs the GMUs read directly (not through a time map)
            mapped = {src for (tgt, maps) in TIME_MAP.items() for src in maps} if model.four_modal else set()
            self.out1g = {n: z(2, B, d) for n in LEVEL1 if n not in mapped}
        # ---- time-axis maps (4-modal only)
        self.tmap: Dict[Tuple[str, str], dict] = {}
        if model.four_modal:
            BD = B * d
            ldbd = pad32(BD)
            for tgt, maps in TIME_MAP.items():
                for src_name, lin in maps.items():
                    Ts, Td = self.N[LEVEL1[src_name][0]], self.N[tgt]
                    To = self.Ng[tgt]                      # output rows computed: all, or rows {0, Td-1}
                    self.tmap[(tgt, src_name)] = dict(lin=lin, Ts=Ts, Td=Td, ldbd=ldbd, h_ct=z(Ts, ldbd, dt=ct), out=z(To, B, d),
                                                      dout=z(To, B, d), dout_ct=z(To, ldbd, dt=ct), dh=z(Ts, B, d))
            self.ones_bd = torch.ones(1, ldbd, device=dev, dtype=ct)
            self.ones_bd[:, BD:] = 0
        # ---- dense Fusion-GMU layers: per target modality a "middle" and a "top" unit
        self.g: Dict[Tuple[str, str], dict] = {}
        for tgt in ("l", "a", "v"):
            R = self.Ng[tgt] * B
            for kind in ("mid", "top"):
                self.g[(tgt, kind)] = dict(R=R, x1=z(R, d), x2=z(R, d), xc=z(R, 2 * self.ld, dt=ct), a1=z(R, d), a2=z(R, d),
                                           ag=z(R, d), out=z(self.Ng[tgt], B, d), da1=z(R, self.ld, dt=ct),
                                           da2=z(R, self.ld, dt=ct), dag=z(R, self.ld, dt=ct), dx1=z(R, d), dx2=z(R, d))
        self._build_gmu()
        self._build_time()
        self._build_sums()
        self._conv_cache = {}
        self._conv: Dict[str, dict] = {}                           # what conv_forward leaves for conv_backward
        self._px_rows: Dict[str, int] = {k: 0 for k in self.N}     # rows of px[k] written by the previous input
        # ---- [B,d] tail (token pick, final n-way GMU, residual head): activations kept for its backward + scratch
        n = 4 if model.four_modal else 3
        Cn = model.out_layer.out_features
        self.tail = dict(n=n, C=Cn, **{k: z(B, n * d) for k in ("x", "z", "t", "dzp", "dtp", "dx")},
                         **{k: z(B, d) for k in ("h", "p1", "y", "dy", "dp1", "dh")}, logits=z(B, Cn),
                         dextra=z(B, d) if n == 4 else None)
        self._tail_desc: Optional[TailDesc] = None                 # what tail_forward leaves for tail_backward
        GraphCache.__init__(self, dev)
        self.stamp = 0                                             # forward passes run (_ModelFn: a backward must be the last one's)

    # -- temporal 1x1 projections (mmtr.py:456-469 / 748-761) -----------------------
    def conv_forward(self, feats: Dict[str, torch.Tensor], seed: int, training: bool) -> None:
        """feats[m]: fp32 [B,T_m,orig_d_m] contiguous.  Fills px[m] = zero-padded [N_m,B,d]."""
        m, B, d, st = self.m, self.B, self.d, self.st
        packs_ct, packs_f32, gemms = [], [], []
        self._conv = {}
        for k in ("l", "a", "v"):
            x = feats[k]
            T, od = x.shape[1], x.shape[2]
            if T > self.N[k]:
                raise ValueError(f"modality {k}: sequence length {T} exceeds num_vectors_{k}={self.N[k]}")
            p = m.embed_dropout if (training and k == "l") else 0.0           # text-feature dropout, mmtr.py:741
            px = self.px[k]
            # rows [T, last) hold an earlier, longer input: clear them (rows past every input so far are still the zeros
            # they were allocated as).  While capturing a graph: always the whole tail -- a replay must leave px right
            # whatever ran before it
            last = self.N[k] if self.capturing else self._px_rows[k]
            if T < last:
                px[T:last].zero_()
            self._px_rows[k] = T
            if od == d:                                                        # projection skipped (mmtr.py:748-750)
                packs_f32.append(ops.pack_problem(B, T, od, d, src=x, dst=px, drop_p=p, drop_site=SITE_TEXT))
                self._conv[k] = dict(T=T, od=od, x=x, p=p, packed=None)
                continue
            kp = pad32(od)
            key = (k, T)
            if key not in self._conv_cache:
                self._conv_cache[key] = dict(packed=torch.zeros(T * B, kp, device=st.device, dtype=ops.ct_torch(self.dtype)),
                                             dy=torch.zeros(T * B, self.ld, device=st.device, dtype=ops.ct_torch(self.dtype)),
                                             dpk=torch.zeros(T * B, od, device=st.device))
            cc = self._conv_cache[key]
            packs_ct.append(ops.pack_problem(B, T, od, kp, src=x, dst=cc["packed"], drop_p=p, drop_site=SITE_TEXT))
            gemms.append(ops.gemm_problem(cc["packed"], st.sptr(f"proj_{k}.weight"), px, T * B, d, od, kp, kp, d))
            self._conv[k] = dict(T=T, od=od, x=x, p=p, **cc)
        if packs_f32:
            ops.pack_rows_fwd(BPM_F32, packs_f32, seed)
        if packs_ct:
            ops.pack_rows_fwd(self.dtype, packs_ct, seed)
            ops.gemm_grouped(self.dtype, GEMM_NT, gemms, seed, x3=self.x3)

    def conv_backward(self, seed: int, need_dx: Dict[str, bool]) -> Dict[str, Optional[torch.Tensor]]:
        """Consumes dpx[m]; accumulates proj_m.weight gradients; returns d(feats[m]) where requested."""
        B, d, st = self.B, self.d, self.st
        casts, wg, dg, unpack = [], [], [], []
        res: Dict[str, Optional[torch.Tensor]] = {"l": None, "a": None, "v": None}
        for k, c in self._conv.items():
            T, od = c["T"], c["od"]
            R = T * B
            if c["packed"] is None:
                if need_dx[k]:
                    res[k] = torch.empty_like(c["x"])
                    unpack.append(ops.pack_problem(B, T, od, 0, g=self.dpx[k], ldg=d, dsrc=res[k], drop_p=c["p"], drop_site=SITE_TEXT))
                continue
            kp = pad32(od)
            casts.append(ops.cast_problem(self.dpx[k], d, R, d, dst_ct=c["dy"], ldd=self.ld))
            wg.append(ops.gemm_problem(c["dy"], c["packed"], st.gptr(f"proj_{k}.weight"), d, od, R, self.ld, kp, od,
                                       flags=F_ACCUM))
            if need_dx[k]:
                res[k] = torch.empty_like(c["x"])
                dg.append(ops.gemm_problem(c["dy"], st.sptr(f"proj_{k}.weight"), c["dpk"], R, od, d, self.ld, kp, od))
                unpack.append(ops.pack_problem(B, T, od, 0, g=c["dpk"], ldg=od, dsrc=res[k], drop_p=c["p"], drop_site=SITE_TEXT))
        if casts:
            ops.rows_cast(self.dtype, casts, seed)
            ops.gemm_grouped(self.dtype, GEMM_TN, wg, seed, x3=self.x3)
        if dg:
            ops.gemm_grouped(self.dtype, GEMM_NN, dg, seed, x3=self.x3)
        if unpack:
            ops.pack_rows_bwd(unpack, seed)
        return res

    # -- time-axis Linear (4-modal) --------------------------------------------------
    def _build_time(self) -> None:
        """Forward: out = W h + bias per map.  Backward: dout (fp32 [Td,B,d], or rows {0, Td-1} of it) of every map ->
        weight / bias gradients and dh (fp32 [Ts,B,d]).  (Exact fp32 products in bf16x3 mode: the tables are not tagged.)"""
        B, d, st = self.B, self.d, self.st
        BD = B * d
        A = ops.array
        casts, gemms, bw_casts, bw_wg, bw_dg = [], [], [], [], []
        for (tgt, src), t in self.tmap.items():
            Ts, Td, ldbd = t["Ts"], t["Td"], t["ldbd"]
            ldw = pad32(Ts)
            W, bias = t["lin"] + ".weight", t["lin"] + ".bias"
            casts.append(ops.cast_problem(self.out1[src], BD, Ts, BD, dst_ct=t["h_ct"], ldd=ldbd))
            bw_casts.append(ops.cast_problem(t["dout"], BD, t["dout"].shape[0], BD, dst_ct=t["dout_ct"], ldd=ldbd))
            if self.prune:
                # output rows {0, Td-1} only: one single-row product each (the row's own bias entry).  Backward: rows
                # {0, Td-1} of the weight / bias gradient (the other rows' are zero: cleared with the small tensors);
                # dh = W[{0, Td-1}]^T dout: k = the two rows, Td-1 apart
                for j, r in enumerate((0, Td - 1)):
                    gemms.append(ops.gemm_problem(st.sptr(W, r * ldw), t["h_ct"], t["out"][j], 1, BD, Ts, ldw, ldbd, BD,
                                                  bias_m=st.p(bias).data_ptr() + 4 * r))
                    bw_wg.append(ops.gemm_problem(t["dout_ct"][j], t["h_ct"], st.gptr(W, r * Ts), 1, Ts, BD, ldbd, ldbd, Ts, flags=F_ACCUM))
                    bw_wg.append(ops.gemm_problem(t["dout_ct"][j], self.ones_bd, st.gptr(bias, r), 1, 1, BD, ldbd, ldbd, 1, flags=F_ACCUM))
                bw_dg.append(ops.gemm_problem(st.sptr(W), t["dout_ct"], t["dh"], Ts, BD, 2, (Td - 1) * ldw, ldbd, BD))
            else:
                gemms.append(ops.gemm_problem(st.sptr(W), t["h_ct"], t["out"], Td, BD, Ts, ldw, ldbd, BD, bias_m=st.p(bias)))
                bw_wg.append(ops.gemm_problem(t["dout_ct"], t["h_ct"], st.gptr(W), Td, Ts, BD, ldbd, ldbd, Ts, flags=F_ACCUM))
                bw_wg.append(ops.gemm_problem(t["dout_ct"], self.ones_bd, st.gptr(bias), Td, 1, BD, ldbd, ldbd, 1, flags=F_ACCUM))
                bw_dg.append(ops.gemm_problem(st.sptr(W), t["dout_ct"], t["dh"], Ts, BD, Td, ldw, ldbd, BD))
        self._time_fwd = (A(CastProblem, casts), A(GemmProblem, gemms))
        self._time_bwd = (A(CastProblem, bw_casts), A(GemmProblem, bw_wg), A(GemmProblem, bw_dg))

    def _time_forward(self) -> None:
        casts, gemms = self._time_fwd
        ops.rows_cast(self.dtype, casts, 0)
        ops.gemm_grouped(self.dtype, GEMM_NN, gemms, 0)

    def _time_backward(self) -> None:
        casts, wg, dg = self._time_bwd
        ops.rows_cast(self.dtype, casts, 0)
        ops.gemm_grouped(self.dtype, GEMM_NT, wg, 0)
        ops.gemm_grouped(self.dtype, GEMM_TN, dg, 0)

    # -- dense Fusion-GMU -------------------------------------------------------------
    def _lvl1(self, tgt: str, name: str) -> torch.Tensor:
        """Level-1 output as the fusion of target `tgt` sees it (through the time map in the 4-modal model)."""
        t = self.tmap.get((tgt, name))
        if t is not None:
            return t["out"]
        return self.out1g[name] if self.prune else self.out1[name]

    def _build_gmu(self) -> None:
        B, d, ld, st = self.B, self.d, self.ld, self.st
        A = ops.array
        casts, gemms, gates = [], [], []
        bw_gate, bw_wg, bw_dg, bw_dg2 = [], [], [], []
        for tgt in ("l", "a", "v"):
            l2a, l1a, l2b, l1b = FUSE[tgt]
            xa, xb = self._lvl1(tgt, l1a), self._lvl1(tgt, l1b)
            for kind, pfx in (("mid", f"gmu_{tgt}_m."), ("top", f"gmu_{tgt}.")):
                g = self.g[(tgt, kind)]
                R = g["R"]
                xc1, xc2 = g["xc"], g["xc"][:, ld:]
                if kind == "mid":
                    casts.append(ops.cast_problem(xa, d, R, d, dst_ct=xc1, ldd=2 * ld, ct_cols=ld, dst_f32=g["x1"], ldf=d))
                    casts.append(ops.cast_problem(xb, d, R, d, dst_ct=xc2, ldd=2 * ld, ct_cols=ld, dst_f32=g["x2"], ldf=d))
                else:                                                       # level 1 -> 2 residual, mmtr.py:799-800
                    casts.append(ops.cast_problem(self.out2[l2a], d, R, d, b=xa, ldb=d, dst_ct=xc1, ldd=2 * ld, ct_cols=ld, dst_f32=g["x1"], ldf=d))
                    casts.append(ops.cast_problem(self.out2[l2b], d, R, d, b=xb, ldb=d, dst_ct=xc2, ldd=2 * ld, ct_cols=ld, dst_f32=g["x2"], ldf=d))
                w1, w2, wg_ = pfx + "hidden1.weight", pfx + "hidden2.weight", pfx + "x_gate.weight"
                gemms.append(ops.gemm_problem(xc1, st.sptr(w1), g["a1"], R, d, d, 2 * ld, ld, d))
                gemms.append(ops.gemm_problem(xc2, st.sptr(w2), g["a2"], R, d, d, 2 * ld, ld, d))
                gemms.append(ops.gemm_problem(xc1, st.sptr(wg_), g["ag"], R, d, 2 * ld, 2 * ld, 2 * ld, d))
                gates.append(ops.gmu_problem(g["a1"], g["a2"], g["ag"], g["x1"], g["x2"], R, out=g["out"]))
                g["dout"] = torch.zeros(self.Ng[tgt], B, d, device=st.device)
                bw_gate.append(ops.gmu_problem(g["a1"], g["a2"], g["ag"], g["x1"], g["x2"], R, dout=g["dout"], da1=g["da1"], da2=g["da2"],
                                               dag=g["dag"], ldg=ld, dx1=g["dx1"], dx2=g["dx2"]))
                bw_wg += [ops.gemm_problem(g["da1"], xc1, st.gptr(w1), d, d, R, ld, 2 * ld, d, flags=F_ACCUM),
                          ops.gemm_problem(g["da2"], xc2, st.gptr(w2), d, d, R, ld, 2 * ld, d, flags=F_ACCUM),
                          ops.gemm_problem(g["dag"], xc1, st.gptr(wg_), d, d, R, ld, 2 * ld, 2 * d, flags=F_ACCUM),
                          ops.gemm_problem(g["dag"], xc2, st.gptr(wg_, d), d, d, R, ld, 2 * ld, 2 * d, flags=F_ACCUM)]
                # dx1 / dx2 already hold the direct terms; the two linear paths are added by two launches
                # (one owner per output tile in each: plain += instead of float atomics)
                bw_dg += [ops.gemm_problem(g["da1"], st.sptr(w1), g["dx1"], R, d, d, ld, ld, d, flags=F_ACCUM),
                          ops.gemm_problem(g["da2"], st.sptr(w2), g["dx2"], R, d, d, ld, ld, d, flags=F_ACCUM)]
                bw_dg2 += [ops.gemm_problem(g["dag"], st.sptr(wg_), g["dx1"], R, d, d, ld, 2 * ld, d, flags=F_ACCUM),
                           ops.gemm_problem(g["dag"], st.sptr(wg_, ld), g["dx2"], R, d, d, ld, 2 * ld, d, flags=F_ACCUM)]
        self._gmu_fwd = (A(CastProblem, casts), A(GemmProblem, gemms), A(GmuProblem, gates))
        self._gmu_bwd = (A(GmuProblem, bw_gate), A(GemmProblem, bw_wg), A(GemmProblem, bw_dg), A(GemmProblem, bw_dg2))
        for arr in (self._gmu_fwd[1],) + self._gmu_bwd[1:]:
            arr.x3 = self.x3                     # bf16x3 mode: eligible launches run as three split-bf16 products

    def gmu_forward(self) -> None:
        casts, gemms, gates = self._gmu_fwd
        ops.rows_cast(self.dtype, casts, 0)
        ops.gemm_grouped(self.dtype, GEMM_NT, gemms, 0)
        ops.gmu2_fwd(gates, self.d)

    def gmu_backward(self) -> None:
        gate, wg, dg, dg2 = self._gmu_bwd
        ops.gmu2_bwd(self.dtype, gate, self.d)
        ops.gemm_grouped(self.dtype, GEMM_TN, wg, 0)
        ops.gemm_grouped(self.dtype, GEMM_NN, dg, 0)
        ops.gemm_grouped(self.dtype, GEMM_NN, dg2, 0)

    # -- whole trunk ------------------------------------------------------------------
    def forward(self, feats: Dict[str, torch.Tensor], seed: int, training: bool) -> List[torch.Tensor]:
        """The caller has refreshed the weight shadows (ParamStore.refresh_shadows: a host-side decision, so it stays
        outside a captured graph)."""
        if self.x3 is not None:
            self.x3.new_step()                       # bf16x3: split images of earlier passes are stale from here on
        self.conv_forward(feats, seed, training)
        px = self.px
        q1 = [px[q] for (q, kv, _) in LEVEL1.values()]
        k1 = [px[kv] for (q, kv, _) in LEVEL1.values()]
        self.plan1.forward(q1, k1, k1, seed, training)
        if self.prune:
            for n, t in self.out1g.items():
                torch.index_select(self.out1[n], 0, self.idx[LEVEL1[n][0]], out=t)
        if self.prune and not self.m.four_modal:
            for k in self.N:
                torch.index_select(px[k], 0, self.idx[k], out=self.pxg[k])
            q2 = [self.pxg[q] for (q, src, _) in LEVEL2.values()]
        else:
            q2 = [px[q] for (q, src, _) in LEVEL2.values()]
        k2 = [self.out1[src] for (q, src, _) in LEVEL2.values()]
        self.plan2.forward(q2, k2, k2, seed, training)
        if self.tmap:
            self._time_forward()
        self.gmu_forward()
        return [self.g[(t, k)]["out"] for t in ("l", "a", "v") for k in ("top", "mid")]

    # -- [B,d] tail -------------------------------------------------------------------
    TAIL_ORDER = ("l", "v", "a")                   # input order of the final GMU (mmtr.py:574, 857)

    def tail_desc(self, extra: Optional[torch.Tensor], training: bool) -> TailDesc:
        m, tl = self.m, self.tail
        t = TailDesc()
        t.B, t.d, t.n, t.C = self.B, self.d, tl["n"], tl["C"]
        for i, k in enumerate(self.TAIL_ORDER):
            t.N[i] = self.Ng[k]
            t.top[i], t.mid[i] = self.g[(k, "top")]["out"].data_ptr(), self.g[(k, "mid")]["out"].data_ptr()
        t.extra = extra.data_ptr() if extra is not None else None
        for i in range(tl["n"]):
            t.Wh[i] = getattr(m.gmu, f"hidden{i + 1}").weight.data_ptr()
            t.Wg[i] = getattr(m.gmu, f"x{i + 1}_gate").weight.data_ptr()
        t.W1, t.b1, t.W2, t.b2 = (x.data_ptr() for x in (m.proj1.weight, m.proj1.bias, m.proj2.weight, m.proj2.bias))
        t.Wo, t.bo = m.out_layer.weight.data_ptr(), m.out_layer.bias.data_ptr()
        t.out_dropout, t.drop_site = (m.out_dropout if training else 0.0), SITE_TEXT + 1
        for k in ("x", "z", "t", "h", "p1", "y", "logits"):
            setattr(t, k, tl[k].data_ptr())
        return t

    def tail_forward(self, extra: Optional[torch.Tensor], seed: int, training: bool):
        self._tail_desc = self.tail_desc(extra, training)
        ops.tail_fwd(self._tail_desc, seed)
        return self.tail["logits"], self.tail["z"]

    def tail_backward(self, dlogits: torch.Tensor, dz: Optional[torch.Tensor], params: Sequence[torch.Tensor]):
        """Writes rows 0 / N-1 of the top / middle GMU output gradients (the trunk's `dout` buffers; their other rows
        are never written and stay zero) and returns the tail parameters' gradients in the order of `params`
        (model.tail_parameters()) plus the gradient of the 4th input."""
        tl, n = self.tail, self.tail["n"]
        gr = TailGrads()
        gr.dlogits = dlogits.data_ptr()
        gr.dz = dz.data_ptr() if dz is not None else None
        flat = torch.zeros(sum((p.numel() + 3) // 4 * 4 for p in params), device=dlogits.device)    # accumulated into (+=) by the kernels
        grads, o = [], 0
        for p in params:
            grads.append(flat[o:o + p.numel()].view(p.shape))
            o += (p.numel() + 3) // 4 * 4
        it = iter(grads)
        for i in range(n):
            gr.dWh[i] = next(it).data_ptr()
        for i in range(n):
            gr.dWg[i] = next(it).data_ptr()
        gr.dW1, gr.db1, gr.dW2, gr.db2, gr.dWo, gr.dbo = (next(it).data_ptr() for _ in range(6))
        for i, k in enumerate(self.TAIL_ORDER):
            gr.dtop[i], gr.dmid[i] = self.g[(k, "top")]["dout"].data_ptr(), self.g[(k, "mid")]["dout"].data_ptr()
        gr.dextra = tl["dextra"].data_ptr() if tl["dextra"] is not None else None
        for k in ("dy", "dp1", "dh", "dzp", "dtp", "dx"):
            setattr(gr, k, tl[k].data_ptr())
        ops.tail_bwd(self._tail_desc, gr)
        return grads, tl["dextra"]

    # -- gradient sums between the levels ------------------------------------------------
    def _build_sums(self) -> None:
        """Grouped bpm_add_n tables of backward(), all operands static.  d(level-2 output) = the top GMU's operand gradient;
        d(level-1 output) = its middle + top GMU operand terms (through the time map where it is consumed through one: summed
        into the map's dout, the term is then the map's dh) + its key / value gradients from level 2; d(projected input) =
        the gradients of every encoder that reads it.  Whole-tensor terms are summed by one grouped launch, two-row terms
        (pruned schedule: rows 0 and N-1) added on top (_rows2_tables)."""
        A, shp = ops.array, lambda k: (self.Ng[k], self.B, self.d)
        whole, rows, d2, to_tmap = {}, {}, {}, []        # level-1 name -> its whole-tensor / two-row GMU terms; level-2 name -> d
        for tgt in ("l", "a", "v"):
            l2a, l1a, l2b, l1b = FUSE[tgt]
            top, mid = self.g[(tgt, "top")], self.g[(tgt, "mid")]
            d2[l2a], d2[l2b] = top["dx1"].view(shp(tgt)), top["dx2"].view(shp(tgt))
            for name, terms in ((l1a, [top["dx1"], mid["dx1"]]), (l1b, [top["dx2"], mid["dx2"]])):
                t = self.tmap.get((tgt, name))
                if t is not None:
                    to_tmap.append(ops.addn_problem(t["dout"], terms))
                    whole[name], rows[name] = [t["dh"]], []
                else:
                    terms = [x.view(shp(tgt)) for x in terms]
                    whole[name], rows[name] = (terms, []) if self.Ng[tgt] == self.N[LEVEL1[name][0]] else ([], terms)
        self._d2 = [d2[n] for n in LEVEL2]
        self._d1 = [self.d1buf[n] for n in LEVEL1]
        # Every encoder gets the same tensor as key and value source: both plans write ONE gradient per source, the fp32
        # sum of the two (EncoderGroupPlan.merge_kv_grads; without the fused key / value source launch they keep two).
        # Level 2's goes straight into d(level-1 output) where no other whole-tensor term joins it there (the pruned
        # 3-modal schedule: the GMU terms are two rows each, added on top afterwards) -- no bpm_add_n for that tensor.
        self.plan2.merge_kv_grads([self.d1buf[src] if not whole[src] else None for (q, src, _) in LEVEL2.values()])
        self.plan1.merge_kv_grads()
        dq2, dk2, dv2 = self.plan2.input_grads()
        sums, rows2 = [], []
        for (n, (q, src, _)), gk, gv in zip(LEVEL2.items(), dk2, dv2):
            d1 = self.d1buf[src]
            rows2 += [(d1, t) for t in rows[src]]
            if gk is not d1:
                sums.append(ops.addn_problem(d1, whole[src] + [g for g in (gk, gv) if g is not None]))
        dq1, dk1, dv1 = self.plan1.input_grads()
        acc: Dict[str, List[torch.Tensor]] = {"l": [], "a": [], "v": []}
        for (n, (q, kv, _)), gq, gk, gv in zip(LEVEL1.items(), dq1, dk1, dv1):
            acc[q].append(gq)
            acc[kv] += [g for g in (gk, gv) if g is not None]
        small: Dict[str, List[torch.Tensor]] = {"l": [], "a": [], "v": []}
        for (n, (q, src, _)), e, gq in zip(LEVEL2.items(), self.plan2.encs, dq2):     # (3-modal pruned schedule: level 2 has
            (small if e.T != self.N[q] else acc)[q].append(gq)                          # two query rows)
        self._sum_tmap = A(AddnProblem, to_tmap)
        self._sum_d1 = A(AddnProblem, sums)
        self._rows2_d1 = self._rows2_tables(rows2)
        self._sum_dpx = A(AddnProblem, [ops.addn_problem(self.dpx[k], terms) for k, terms in acc.items()])
        self._rows2_dpx = self._rows2_tables([(self.dpx[k], gq) for k in acc for gq in small[k]])

    def _rows2_tables(self, pairs):
        """dst[0] += t[0], dst[N-1] += t[1] for (dst [N, B, d], t [2, B, d]) pairs as grouped bpm_add_n launches over the row
        blocks (in place, terms added in list order: the result index_add_ per term gave, which was 18 launches of 5 us and
        as many dependency gaps per step at hidden 768).  Returns (launch tables, pairs left to torch: unaligned blocks)."""
        if (self.B * self.d) % 4:
            return [], pairs
        terms: Dict[tuple, list] = {}
        for dst, t in pairs:
            for j, r in ((0, 0), (1, dst.shape[0] - 1)):
                terms.setdefault((dst.data_ptr(), r), [dst[r]]).append(t[j])
        launches = []
        while terms:                                      # at most 8 inputs per problem (the destination among them), and a
            probs = []                                    # destination once per launch
            for key in list(terms):
                out, ins = terms[key][0], terms[key][1:]
                probs.append(ops.addn_problem(out, [out] + ins[:7]))
                if len(ins) > 7:
                    terms[key] = [out] + ins[7:]
                else:
                    del terms[key]
            launches.append(ops.array(AddnProblem, probs))
        return launches, []

    @staticmethod
    def _add_rows2(tables) -> None:
        launches, pairs = tables
        for arr in launches:
            ops.add_n(arr)
        for dst, t in pairs:
            dst[0] += t[0]
            dst[-1] += t[1]

    def backward(self, seed: int, need_dx: Dict[str, bool], stores: Optional[bool] = None):
        """The `dout` buffers of the GMU units hold d(top_l), d(mid_l), ... (written by tail_backward).  When the gradients
        are unset (zero_grad / `p.grad = None`) the flat gradient buffer is NOT cleared as a whole: the encoders' large
        weight gradients are written by their first launch (`stores` launch tables) and one table-driven launch clears the
        rest.  stores given (captured graphs: part of the graph's key): the caller attaches the .grad views afterwards."""
        st = self.st
        attach = stores is None
        if stores is None:
            stores = st.begin_backward(stores=True)
        elif stores:
            ops.zero_segments(*st._zero_table)
        self.gmu_backward()
        if self.tmap:
            ops.add_n(self._sum_tmap)
            self._time_backward()
        self._ready("fuse")
        self.plan2.backward(self._d2, self._layer_hook("level2"), stores=stores)
        ops.add_n(self._sum_d1)
        self._add_rows2(self._rows2_d1)
        self.plan1.backward(self._d1, self._layer_hook("level1"), stores=stores)
        ops.add_n(self._sum_dpx)
        self._add_rows2(self._rows2_dpx)
        res = self.conv_backward(seed, need_dx)
        self._ready("proj")
        if attach:
            st.end_backward()
        return res

    # -- captured launch sequences (GraphCache.replay) ------------------------------------
    def graph_forward(self, feats: Dict[str, torch.Tensor], extra: Optional[torch.Tensor], seed: int, training: bool):
        """Forward pass through a captured graph when one exists (or can be captured now) for this key; returns
        (logits, z, key) or None (the caller then runs eagerly)."""
        key = (training, tuple(tuple(feats[k].shape) for k in ("l", "v", "a")), extra is not None)

        def run(static, handle):
            self.forward(static, handle, training)
            return self.tail_forward(static["extra"], handle, training)

        ent = self.replay(True, key, seed, {k: feats[k] for k in ("l", "v", "a")} | {"extra": extra}, run,
                              f"BPMulT: graph capture of the forward pass failed for input shapes {key[1]} (%s); "
                              "this shape runs as eager launches",
                              on_fail=lambda: self._px_rows.update(self.N))    # nothing of the capture ran: clear the pad rows again
        if ent is None:
            return None
        if "state" not in ent:    # host-side state a forward leaves for its backward (a replay runs no Python): restored
            ent["state"] = (self._conv, self._tail_desc, self.plan1._last, self.plan2._last)      # before the backward
        self.plan1.maps_ready()                      # (no Python of EncoderGroupPlan.forward ran: attention_maps)
        self.plan2.maps_ready()
        self._px_rows = {k: feats[k].shape[1] for k in ("l", "v", "a")}
        return ent["out"][0], ent["out"][1], key

    def graph_backward(self, fkey, dlogits: torch.Tensor, dz: Optional[torch.Tensor], params, seed: int, need: Dict[str, bool]):
        """Backward of a graph-run forward.  Whether the gradients start from zero (first-writer-stores launch tables +
        the small tensors cleared) or accumulate is part of the key.  Returns (parameter gradients of the tail, d(extra),
        d(features)) as clones of the graph's static outputs, or None before the key is captured (or when its capture
        failed: the caller runs the eager backward -- the forward state has been restored)."""
        self._conv, self._tail_desc, self.plan1._last, self.plan2._last = self._fg[fkey]["state"]
        fresh = self.st._fresh()
        key = (fkey, fresh, dz is not None, tuple(sorted(k for k, v in need.items() if v)))

        def run(static, handle):
            pg, dextra = self.tail_backward(static["dlogits"], static["dz"], params)
            return pg, dextra, self.backward(handle, need, stores=fresh)

        ent = self.replay(False, key, seed, {"dlogits": dlogits, "dz": dz}, run,
                              "BPMulT: graph capture of the backward pass failed (%s); this key runs as eager launches")
        if ent is None:
            return None
        self.st.end_backward()
        pg, dextra, res = ent["out"]
        return [t.clone() for t in pg], dextra, {k: (v.clone() if v is not None else None) for k, v in res.items()}

    def _ready(self, section: str, events=None) -> None:
        hook = getattr(self.m, "_grad_ready_hook", None)
        if hook is not None:
            lo, hi = self.st.sections[section]
            if hi > lo:
                hook(self.st.gflat, lo, hi, events)

    def _layer_hook(self, tag: str):
        if getattr(self.m, "_grad_ready_hook", None) is None:
            return None
        top = self.m.layers - 1

        def on_layer(i: int, events) -> None:
            if i == top:                                  # the final LayerNorm's gradients were written before layer top
                self._ready(f"{tag}.final", events)
            self._ready(f"{tag}.layer{i}", events)
        return on_layer


class _ModelFn(torch.autograd.Function):
    """The whole hot path as ONE autograd node: temporal projections, the twelve encoders, the Fusion-GMU units and the
    [B,d] tail.  Inputs that can need a gradient: the three feature tensors, the optional 4th fusion input (poster
    projection output) and the tail's parameters (PyTorch-owned; the trunk's live in the flat store)."""

    @staticmethod
    def forward(ctx, anchor, x_l, x_v, x_a, extra, model, *tail_params):
        trunk = model._trunk_for(x_l.shape[0])
        seed = model._next_seed()
        feats = {"l": x_l.detach().contiguous(), "v": x_v.detach().contiguous(), "a": x_a.detach().contiguous()}
        ex = extra.detach().contiguous() if extra is not None else None
        trunk.st.refresh_shadows()
        ran = trunk.graph_forward(feats, ex, seed, model.training) if model._graphs_on() else None
        if ran is None:
            trunk.forward(feats, seed, model.training)
            logits, z = trunk.tail_forward(ex, seed, model.training)
            ctx.fkey = None
        else:
            logits, z, ctx.fkey = ran
        trunk.stamp += 1
        model._last_trunk = trunk
        ctx.trunk, ctx.seed, ctx.stamp, ctx.extra, ctx.params = trunk, seed, trunk.stamp, ex, tail_params
        ctx.need = {"l": x_l.requires_grad, "v": x_v.requires_grad, "a": x_a.requires_grad}
        return logits.detach().clone(), z.detach().clone()

    @staticmethod
    def backward(ctx, dlogits, dz):
        if ctx.stamp != ctx.trunk.stamp:
            # activations live in per-batch-size buffers owned by the model, not in the autograd graph
            raise RuntimeError("BPMulT hot path: backward() of a forward pass that a later forward pass (same model, same "
                               "batch size) has overwritten; run forward -> backward one step at a time")
        dlogits = dlogits.contiguous().float()
        dz = dz.contiguous().float() if dz is not None else None
        ran = ctx.trunk.graph_backward(ctx.fkey, dlogits, dz, ctx.params, ctx.seed, ctx.need) if ctx.fkey is not None else None
        if ran is not None:
            pgrads, dextra, res = ran
        else:
            pgrads, dextra = ctx.trunk.tail_backward(dlogits, dz, ctx.params)
            res = ctx.trunk.backward(ctx.seed, ctx.need)
        return (None, res["l"], res["v"], res["a"], dextra.clone() if (dextra is not None and ctx.extra is not None) else None,
                None) + tuple(pgrads)


class _BPMulTBase(nn.Module):
    four_modal = False

    def _init_common(self, args):
        self.args = args
        self.orig_d_l, self.orig_d_v, self.orig_d_a = args.orig_d_l, args.orig_d_v, args.orig_d_a
        self.d = self.d_l = self.d_a = self.d_v = args.hidden_sz
        self.vonly, self.lonly, self.aonly = args.vonly, args.lonly, args.aonly
        if not (self.vonly and self.lonly and self.aonly):
            raise NotImplementedError("the hot path is built for the full model (lonly = vonly = aonly = True, the default)")
        if getattr(args, "hybrid", False):
            raise NotImplementedError("--hybrid is broken in the reference (SURVEY.md section 0) and outside the hot path")
        self.num_heads, self.layers = args.num_heads, args.layers
        self.attn_dropout, self.attn_dropout_v, self.attn_dropout_a = args.attn_dropout, args.attn_dropout_v, args.attn_dropout_a
        self.relu_dropout, self.res_dropout = args.relu_dropout, args.res_dropout
        self.out_dropout, self.embed_dropout, self.attn_mask = args.out_dropout, args.embed_dropout, args.attn_mask
        self.precision: Optional[str] = getattr(args, "precision", None)
        # exact dead-row elimination (see _Trunk): ON by default -- same logits, gates and gradients as the
        # reference's dense schedule (pinned against the reference fixtures in both schedules, tests/test_model_gpu.py).
        # `args.prune_unused_rows=False`, `set_prune_unused_rows(False)` or BPMULT_PRUNE=0 run the dense schedule.
        flag = getattr(args, "prune_unused_rows", None)
        self.prune_unused_rows = (os.environ.get("BPMULT_PRUNE", "1") != "0") if flag is None else bool(flag)
        # deterministic mode (config.set_deterministic): None = the process default, read when a trunk's tables are built
        flag = getattr(args, "deterministic", None)
        self.deterministic: Optional[bool] = None if flag is None else bool(flag)
        d = self.d
        self.enc = BertEncoder(args)
        self.enc.store_prefix = "enc."
        for t in ("l", "v", "a"):
            setattr(self, f"gmu_{t}_m", GatedMultimodalLayerFeatures(d, d, d))
        for t in ("l", "v", "a"):
            setattr(self, f"gmu_{t}", GatedMultimodalLayerFeatures(d, d, d))
        self.proj_l = nn.Conv1d(self.orig_d_l, d, kernel_size=1, padding=0, bias=False)
        self.proj_v = nn.Conv1d(self.orig_d_v, d, kernel_size=1, padding=0, bias=False)
        self.proj_a = nn.Conv1d(self.orig_d_a, d, kernel_size=1, padding=0, bias=False)
        tag_drop = {"l": self.attn_dropout, "a": self.attn_dropout_a, "v": self.attn_dropout_v}
        order = ["trans_l_with_a", "trans_l_with_v", "trans_l_with_v2a", "trans_l_with_a2v",
                 "trans_v_with_l", "trans_v_with_a", "trans_v_with_l2a", "trans_v_with_a2l",
                 "trans_a_with_l", "trans_a_with_v", "trans_a_with_v2l", "trans_a_with_l2v"]       # reference registration order
        for n in order:
            key = (LEVEL1.get(n) or LEVEL2.get(n))[2]
            setattr(self, n, TransformerEncoder(d, self.num_heads, self.layers, attn_dropout=tag_drop[key],
                                                relu_dropout=self.relu_dropout, res_dropout=self.res_dropout,
                                                embed_dropout=self.embed_dropout, attn_mask=self.attn_mask,
                                                biprojection=self.four_modal and n in LEVEL2))
        self.proj1, self.proj2 = nn.Linear(d, d), nn.Linear(d, d)
        self.out_layer = nn.Linear(d, args.n_classes)
        self._store: Optional[ParamStore] = None
        self._trunks: Dict[int, _Trunk] = {}
        # host-side step counter of the dropout stream; FusedAdam.state_dict() carries it (the model's state_dict keys
        # stay exactly the reference's), so a resumed run continues the mask sequence
        self.dropout_step = 0

    def _init_time_maps(self):
        L, A, V = self.num_vectors_l, self.num_vectors_a, self.num_vectors_v
        self.transfm_a2l, self.transfm_v2l = nn.Linear(A, L), nn.Linear(V, L)
        self.transfm_l2a, self.transfm_l2v = nn.Linear(L, A), nn.Linear(L, V)

    # -- engine plumbing -------------------------------------------------------------
    TAIL = ("enc.", "audio_enc.", "proj_poster.", "gmu.", "proj1.", "proj2.", "out_layer.")

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._drop_trunks()
        self._store = None
        return r

    def attention_maps(self, names=None, layers=None, per_head: bool = False):
        """Head-averaged attention maps of the most recent forward call: a dict from encoder name (the reference's
        attribute names, "trans_l_with_a", ..., "trans_v_with_a2l"; `names` = None: all twelve) to a list with one entry
        per selected layer (`layers` = None: all), each a dict from attention block to engine.AttentionMap(weights,
        query_steps): {"cross": [B, Tq, S]} for a crossmodal encoder, {"self": [B, Tq, T], "cross": [B, Tq, S]} for the
        4-modal model's biprojection level-2 encoders.  These are what forward hooks on `<encoder>.layers[i].self_attn`
        read off the reference (second return value, multihead_attention.py:132-135): the softmax probabilities averaged
        over the heads, BEFORE attention dropout -- equal to the reference's in eval mode and whenever the attention
        dropout rate is 0 (in training with dropout the reference returns the dropped, rescaled matrix) -- exactly 0 at
        masked keys, detached (no gradient flows through them; the reference's layers discard them).

        Under dead-row elimination (the default schedule) some layers only compute two query rows: their maps have
        Tq = 2 and query_steps == (0, N - 1) (the rows' time steps); otherwise query_steps is None and Tq = N.  All maps of
        the headline model are 12 x 8 maps of 8 MB: select with `names` / `layers` -- nothing is computed for the rest,
        and nothing at all unless this is called (the step itself is unchanged).  Works in both schedules, after eager
        launches and after a graph replay (the maps launch itself is never captured), in train and eval mode, under
        no_grad or not, before or after backward(), until the next forward call of this model; RuntimeError before the
        first forward and after .to() / set_prune_unused_rows() dropped the activation buffers.

        per_head=True: every head's probabilities instead of their mean -- weights [B, H, Tq, S] ([B, H, 2, S] for the two-row
        layers), query_steps unchanged, same key masks, same rules.  One full map is then B * H * 512 * 512 * 4 bytes, about
        100 MB at the headline shape, and all maps of a model run to several GB: select `names` and `layers`."""
        trunk = getattr(self, "_last_trunk", None)
        if trunk is None:
            raise RuntimeError("attention_maps: no forward pass to take the maps of (call forward first; .to() and "
                               "set_prune_unused_rows() drop the activation buffers)")
        names = list(ENC_ORDER) if names is None else list(names)
        for n in names:
            if n not in ENC_ORDER:
                raise ValueError(f"attention_maps: unknown encoder {n!r}; the encoders are {ENC_ORDER}")
        L = self.layers
        for i in (range(L) if layers is None else layers):
            if not isinstance(i, int) or not 0 <= i < L:
                raise IndexError(f"attention_maps: layer {i!r} out of range ({L} layers)")
        out = {}
        for plan, level in ((trunk.plan1, LEVEL1), (trunk.plan2, LEVEL2)):
            sel = [n for n in names if n in level]
            if sel:
                out.update(zip(sel, plan.attention_maps(sel, layers, per_head)))
        return {n: out[n] for n in names}

    def _drop_trunks(self) -> None:
        self._last_trunk = None
        for t in getattr(self, "_trunks", {}).values():
            t.retire_graphs()
        self._trunks = {}

    def __del__(self):
        try:
            self._drop_trunks()
        except Exception:                  # noqa: BLE001 -- interpreter shutdown
            pass

    def _ensure_store(self) -> ParamStore:
        if self._store is None or not self._store.still_flat():
            allp = {n: p for n, p in self.named_parameters() if not n.startswith(self.TAIL)}
            # flat layout in reverse execution order, so a finished section of the gradient buffer
            # can be all-reduced while backward continues (distributed.GradSync)
            # ... at LAYER granularity inside a level: the six encoders run their layers in lock-step, so layer i
            # of all six is one contiguous ~26 MB slice that is final ~2 layers after backward passes it
            def lvl(names, tag):
                out = [(f"{tag}.final", lambda n, names=names: n.split(".")[0] in names and n.split(".")[1] == "layer_norm")]
                for i in reversed(range(self.layers)):
                    out.append((f"{tag}.layer{i}", lambda n, names=names, i=i: n.split(".")[0] in names
                                and n.split(".")[1] == "layers" and int(n.split(".")[2]) == i))
                return out
            secs = ([("fuse", lambda n: n.startswith(("gmu_", "transfm_")))] + lvl(LEVEL2, "level2") + lvl(LEVEL1, "level1")
                    + [("proj", lambda n: n.startswith("proj_"))])
            named, bounds = [], []
            for sname, pred in secs:
                part = [(n, p) for n, p in allp.items() if pred(n)]
                bounds.append((sname, len(named), len(named) + len(part)))
                named += part
            assert len(named) == len(allp), "every trunk parameter belongs to exactly one section"
            prec = self.precision or config.precision()
            dt = config.dtype_code(prec)
            st = ParamStore(named, dt, x3=config.is_x3(prec))
            st.sections = {}
            for sname, a, b in bounds:
                lo = st.off[named[a][0]] if b > a else 0
                hi = (st.off[named[b][0]] if b < len(named) else st.total) if b > a else 0
                st.sections[sname] = (lo, hi)
            d = self.d
            for n in ENC_ORDER:
                register_encoder_shadows(st, n + ".", d, self.layers, biprojection=self.four_modal and n in LEVEL2)
            for k, od in (("l", self.orig_d_l), ("v", self.orig_d_v), ("a", self.orig_d_a)):
                st.add_shadow(f"proj_{k}.weight", f"proj_{k}.weight", d, od)
            ld = pad32(d)
            for t in ("l", "v", "a"):
                for pfx in (f"gmu_{t}_m.", f"gmu_{t}."):
                    st.add_shadow(pfx + "hidden1.weight", pfx + "hidden1.weight", d, d)
                    st.add_shadow(pfx + "hidden2.weight", pfx + "hidden2.weight", d, d)
                    # x_gate [d, 2d] -> [d, 2*ld]: each half padded on its own so it lines up with [x1 | x2]
                    st.add_shadow(pfx + "x_gate.weight", pfx + "x_gate.weight", d, d, src_ld=2 * d, dst_ld=2 * ld)
                    st.add_shadow(pfx + "x_gate.weight#2", pfx + "x_gate.weight", d, d, src_col0=d, src_ld=2 * d, dst_ld=2 * ld,
                                  dst_col0=ld, base_key=pfx + "x_gate.weight")
            if self.four_modal:
                for lin in ("transfm_a2l", "transfm_v2l", "transfm_l2a", "transfm_l2v"):
                    w = getattr(self, lin).weight
                    st.add_shadow(lin + ".weight", lin + ".weight", w.shape[0], w.shape[1])
            st.finalize_shadows()
            st.set_store_written([w for n in ENC_ORDER for w in EncoderGroupPlan.store_written(n + ".", self.layers)])
            self._drop_trunks()
            self._store = st
            self._anchor = torch.zeros(1, device=st.device, requires_grad=True)
        return self._store

    def _flat_stores(self) -> List[ParamStore]:
        """Every flat parameter store of the model: [trunk store], and behind it the text encoder's with
        `args.text_params = "flat"`.  What FusedAdam steps in one launch and GradSync exchanges in place."""
        stores = [self._ensure_store()]
        self.enc.precision = self.precision
        text = self.enc.flat_store()
        if text is not None:
            stores.append(text)
        return stores

    MAX_TRUNKS = 2          # activation buffer sets kept (one per batch size, multi-GB each): most recently used

    def _trunk_for(self, B: int) -> _Trunk:
        self._ensure_store()
        t = self._trunks.pop(B, None)
        if t is None:
            while len(self._trunks) >= self.MAX_TRUNKS:
                self._trunks.pop(next(iter(self._trunks))).retire_graphs()         # least recently used
            t = _Trunk(self, B)
        self._trunks[B] = t                                         # (re)insert as most recent
        return t

    def set_prune_unused_rows(self, flag: bool) -> None:
        """Switch between the dense schedule (the reference's) and exact dead-row elimination (the default: level-2 /
        Fusion-GMU / time-map work on rows {0, N-1} only where nothing else is consumed; same logits and gradients,
        SURVEY A.10).  Launch tables are rebuilt on the next forward."""
        self.prune_unused_rows = bool(flag)
        self._drop_trunks()

    def set_deterministic(self, flag: Optional[bool]) -> None:
        """Deterministic mode for this model (None: follow config.deterministic()): no launch of the trunk adds floats in
        hardware order, so a fixed build, device, input and seed give the same bits on every run ("Deterministic
        mode").  Launch tables and captured graphs are rebuilt on the next forward."""
        self.deterministic = None if flag is None else bool(flag)
        self.enc.deterministic = self.deterministic
        self._drop_trunks()

    def _next_seed(self) -> int:
        """Dropout seed of the next forward pass: (process seed, data-parallel rank, step).  Ranks that seed alike
        must still draw independent masks on their shards, as the reference's DataParallel replicas do; the step
        counter is saved with the optimizer state (FusedAdam.state_dict) so a resumed run does not
        replay the mask sequence from step 1."""
        self.dropout_step += 1
        return step_seed(self.dropout_step)

    def _graphs_on(self) -> bool:
        """Captured-graph replay of the step (_Trunk.graph_forward, graphs.GraphCache): on unless switched off (`use_graphs`,
        BPMULT_GRAPH=0), a gradient-exchange hook needs the eager launch order, or the launch profiler is recording."""
        if not getattr(self, "use_graphs", True) or os.environ.get("BPMULT_GRAPH", "1") == "0":
            return False
        if getattr(self, "_grad_ready_hook", None) is not None:
            return False
        from .. import _lib
        return not _lib.prof_enabled()

    def _encode_text(self, txt, mask, segment):
        """self.enc(...); a HIP text encoder runs at the model's precision and draws its dropout masks from the step the
        trunk is about to take (the counter FusedAdam.state_dict carries)."""
        self.enc.precision = self.precision
        self.enc.dropout_step = self.dropout_step
        hook = getattr(self, "_grad_ready_hook", None)
        # all text work is on the current stream: a section is final once everything launched so far has run (events None)
        self.enc._grad_ready = (lambda flat, lo, hi: hook(flat, lo, hi, None)) if hook is not None else None
        return self.enc(txt, mask, segment)

    def tail_parameters(self):
        """The [B,d] tail's parameters in the order bpm_tail_bwd's gradients are returned."""
        n = self.gmu.n
        return ([getattr(self.gmu, f"hidden{i + 1}").weight for i in range(n)] + [getattr(self.gmu, f"x{i + 1}_gate").weight for i in range(n)]
                + [self.proj1.weight, self.proj1.bias, self.proj2.weight, self.proj2.bias, self.out_layer.weight, self.out_layer.bias])

    def _run(self, x_l, x_v, x_a, extra):
        """features -> (logits, gates) through the HIP path (one autograd node)."""
        self._ensure_store()
        tail = self.tail_parameters()
        for p in tail:
            if p.dtype != torch.float32 or not p.is_contiguous():
                raise RuntimeError("BPMulT tail parameters must be contiguous float32")
        return _ModelFn.apply(self._anchor, x_l.float(), x_v.float(), x_a.float(), extra.float() if extra is not None else None,
                              self, *tail)


class MultiprojectionMMTransformer3DGMUClf(_BPMulTBase):
    """3-modal BPMulT (text, video, audio).  forward(txt, mask, segment, img, audio, output_gate=False)."""
    four_modal = False

    def __init__(self, args):
        super().__init__()
        self._init_common(args)
        d = self.d
        self.gmu = TextShiftingLayer([d, d, d], d)
        # sequence lengths are source constants in the reference (mmtr.py:664-670); overridable here
        self.num_vectors_l = getattr(args, "num_vectors_l", 512)
        self.num_vectors_a = getattr(args, "num_vectors_a", 512)
        self.num_vectors_v = getattr(args, "num_vectors_v", 512)
        self._init_time_maps()            # present in the state_dict, unused by the 3-modal graph (mmtr.py:794-795)

    def forward(self, txt, mask, segment, img, audio, output_gate=False):
        x_l = self._encode_text(txt, mask, segment)            # [B,L,orig_d_l]
        logits, z = self._run(x_l, img, audio, None)
        return (logits, z) if output_gate else logits


class MultiprojectionMMTransformerGMUClf(_BPMulTBase):
    """4-modal BPMulT (text, video, audio, poster).  forward(txt, mask, segment, img, audio, poster, output_gate=False)."""
    four_modal = True

    def __init__(self, args):
        super().__init__()
        self.orig_d_p = args.orig_d_p
        self._init_common(args)
        d = self.d
        self.audio_enc = AudioEncoder(args)
        self.proj_poster = nn.Linear(self.orig_d_p, d, bias=False)
        self.gmu = TextShiftingLayer([d, d, d, d], d)
        self.num_vectors_l = getattr(args, "num_vectors_l", 512)
        self.num_vectors_a = getattr(args, "num_vectors_a", 200)
        self.num_vectors_v = getattr(args, "num_vectors_v", 200)
        self._init_time_maps()

    def forward(self, txt, mask, segment, img, audio, poster, output_gate=False):
        from ..frontend import skinny_linear
        prec = self.precision or config.precision()
        x_l = self._encode_text(txt, mask, segment)
        x_a = self.audio_enc.encode(audio, prec)               # [B,96,T_a] -> [B,A,96] (mmtr.py:449)
        logits, z = self._run(x_l, img, x_a, skinny_linear(poster, self.proj_poster.weight, prec))
        return (logits, z) if output_gate else logits
