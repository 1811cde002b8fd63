"""`TransformerEncoder` with the reference's constructor, forward signature and
state_dict layout (bpmult/models/transformer.py:9-99), executed by the grouped
HIP engine.  The sub-modules below are parameter containers that reproduce the
reference's parameter names; none of them has a PyTorch forward
(MultiheadAttention, models/attention.py, has a HIP forward of its own that the
encoder never calls).
"""
from __future__ import annotations

import math
from typing import Optional

import torch
from torch import nn

from .. import config
from ..engine import EncoderDesc, EncoderGroupPlan, EncoderMasks, GroupCfg, ParamStore, register_encoder_shadows
from .attention import MultiheadAttention          # a parameter container here: the encoder runs its own engine plan


def _xavier_linear(i: int, o: int) -> nn.Linear:
    m = nn.Linear(i, o)
    nn.init.xavier_uniform_(m.weight)                         # transformer.py:219-224
    nn.init.constant_(m.bias, 0.0)
    return m


class TransformerEncoderLayer(nn.Module):
    def __init__(self, embed_dim: int, num_heads: int, attn_dropout: float, biprojection: bool):
        super().__init__()
        self.self_attn = MultiheadAttention(embed_dim, num_heads, attn_dropout)
        self.fc1 = _xavier_linear(embed_dim, 4 * embed_dim)
        self.fc2 = _xavier_linear(4 * embed_dim, embed_dim)
        self.layer_norms = nn.ModuleList([nn.LayerNorm(embed_dim) for _ in range(3 if biprojection else 2)])


class SinusoidalPositionalEmbedding(nn.Module):
    """Only the reference's buffer (position_embedding.py:42); the table itself is
    built by engine.sinusoid_table and gathered inside the embedding kernel."""

    def __init__(self, embedding_dim: int):
        super().__init__()
        self.embedding_dim = embedding_dim
        self.register_buffer("_float_tensor", torch.zeros(1))


class _EncoderFn(torch.autograd.Function):
    @staticmethod
    def forward(ctx, anchor, x_q, x_k, x_v, enc, epm=None, kpm=None):
        """x_k / x_v None: the self-attention stack (the encoder's self-only plan; its only input is x_q).  epm / kpm: the
        padding masks of x_q's rows / of the key / value source's rows (TransformerEncoder.forward), or None."""
        plan = enc._plan_for(x_q, x_k, epm is not None, kpm is not None)
        enc._store.refresh_shadows()
        if plan.x3 is not None:
            plan.x3.new_step()
        kv = ([None], [None]) if x_k is None else ([x_k.detach().contiguous()], [x_v.detach().contiguous()])
        masks = {} if epm is None and kpm is None else dict(self_masks=[epm], cross_masks=[kpm])
        out = plan.forward([x_q.detach().contiguous()], *kv, enc._next_seed(), enc.training, **masks)[0]
        ctx.enc, ctx.plan = enc, plan
        enc._last_plan = plan
        return out.detach().clone()

    @staticmethod
    def backward(ctx, dout):
        enc, plan = ctx.enc, ctx.plan
        enc._store.begin_backward()
        dq, dk, dv = plan.backward([dout])
        enc._store.end_backward()
        if dk[0] is None:
            return None, dq[0].clone(), None, None, None, None, None
        return None, dq[0].clone(), dk[0].clone(), dv[0].clone(), None, None, None


class TransformerEncoder(nn.Module):
    """Drop-in for bpmult.models.transformer.TransformerEncoder.

    forward(x_in, x_in_k, x_in_v) on [T,B,d] / [S,B,d] fp32 CUDA tensors: the crossmodal call (the biprojection layer
    kind: self-attention, then attention over x_in_k / x_in_v).  forward(x_in), or any call with x_in_k or x_in_v None
    (the reference's condition, transformer.py:71,84): the self-attention stack over x_in's own T time steps, [T,B,d].
    In the biprojection layer kind that stack follows the reference's layer exactly: its FFN is normalised by
    layer_norms.2, and layer_norms.1 (maybe_layer_norm(1, after=True), the identity) gets no gradient -- it ends zero.
    Both call forms run on the HIP engine and share one parameter store; plans are kept per call form, shape and which
    padding masks the call carries.

    Padding masks (keyword-only; the reference's docstrings promise an encoder_padding_mask, transformer.py:62-63, :145-146,
    and never implement one): torch.bool or torch.uint8 tensors on the inputs' device, any strides, nonzero / True =
    padding, no gradient.
      encoder_padding_mask [B, T]  the padding rows of x_in: hidden as KEYS of every self-attention block -- forward(x) of
                                   either layer kind, and the self-attention block of the biprojection crossmodal call.  No
                                   block of the plain crossmodal call would read it: ValueError there.
      key_padding_mask [B, S]      the padding rows of x_in_k / x_in_v: hidden as keys of the cross-attention block.
                                   ValueError in the self-attention call form, which has no key source.
    A hidden key gets probability exactly 0 for every head and query row of its sample, ANDed with the future-mask rule
    under attn_mask=True: d(x_in_k) / d(x_in_v) rows of padded positions are exactly 0, and in the self-attention forms a
    padded row of x_in whose upstream gradient is 0 has d(x_in) exactly 0.  Query rows are never masked: the output rows
    of padded query positions are computed like any other row, finite and unspecified.  Every query row of every sample
    must keep a visible key under all rules together (not checked: the masks never travel to the host; NaN otherwise).
    Right padding with at least one real row always satisfies it, under the causal rule too: key 0 is visible to every
    row whenever mask_off >= 1.  Precisions 'bf16', 'f32' and 'bf16x3' (whose attention runs the f32 entries).
    attention_maps() after a masked forward is taken under the same masks: exactly 0 at padded keys."""

    def __init__(self, embed_dim, num_heads, layers, attn_dropout=0.0, relu_dropout=0.0, res_dropout=0.0,
                 embed_dropout=0.0, attn_mask=False, biprojection=False):
        super().__init__()
        self.dropout = embed_dropout
        self.attn_dropout, self.relu_dropout, self.res_dropout = attn_dropout, relu_dropout, res_dropout
        self.embed_dim, self.num_heads = embed_dim, num_heads
        self.embed_scale = math.sqrt(embed_dim)
        self.embed_positions = SinusoidalPositionalEmbedding(embed_dim)
        self.attn_mask, self.biprojection = attn_mask, biprojection
        self.layers = nn.ModuleList([TransformerEncoderLayer(embed_dim, num_heads, attn_dropout, biprojection)
                                     for _ in range(layers)])
        self.register_buffer("version", torch.Tensor([2]))
        self.normalize = True
        self.layer_norm = nn.LayerNorm(embed_dim)
        self.precision: Optional[str] = None          # None -> config.precision() at first use
        self.deterministic: Optional[bool] = None     # None -> config.deterministic(), read when a plan is built
        self._store: Optional[ParamStore] = None
        self._plans = {}
        self._last_plan: Optional[EncoderGroupPlan] = None      # plan of the most recent forward call (attention_maps)
        self._step = 0

    def group_cfg(self, self_only: bool = False) -> GroupCfg:
        return GroupCfg(self.embed_dim, self.num_heads, len(self.layers), self.relu_dropout, self.res_dropout, self.dropout,
                        self.attn_mask, self.biprojection, self_only=self_only)

    # -- standalone execution (a group of one) ----------------------------------
    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._store, self._plans, self._last_plan = None, {}, None
        return r

    def _ensure_store(self) -> ParamStore:
        if self._store is None or not self._store.still_flat():
            prec = self.precision or config.precision()
            self._store = ParamStore(list(self.named_parameters()), config.dtype_code(prec), x3=config.is_x3(prec))
            register_encoder_shadows(self._store, "", self.embed_dim, len(self.layers), biprojection=self.biprojection)
            self._store.finalize_shadows()
            self._plans, self._last_plan = {}, None
            self._anchor = torch.zeros(1, device=self._store.device, requires_grad=True)
        return self._store

    def _plan_for(self, x_q, x_k, epm: bool = False, kpm: bool = False) -> EncoderGroupPlan:
        """x_k None: the self-attention-only plan of x_q's shape.  epm / kpm: the call carries an encoder_padding_mask / a
        key_padding_mask -- a plan of its own (a call without masks reaches the plan, under the key, it always did)."""
        st = self._ensure_store()
        T, B = x_q.shape[0], x_q.shape[1]
        key = ("self", T, B) if x_k is None else (T, x_k.shape[0], B)
        if epm or kpm:
            key += ("masks", epm, kpm)
        det = config.resolve_deterministic(self.deterministic)
        if det:
            key += ("det",)
        if key not in self._plans:
            S = T if x_k is None else x_k.shape[0]
            desc = EncoderDesc("", 0, T, S, self.attn_dropout)
            masks = dict(masks=[EncoderMasks(self_keys=epm, cross_keys=kpm)]) if epm or kpm else {}
            self._plans[key] = EncoderGroupPlan(st, self.group_cfg(self_only=x_k is None), [desc], B, deterministic=det, **masks)
        return self._plans[key]

    def _next_seed(self) -> int:
        self._step += 1
        return (torch.initial_seed() * 1000003 + self._step) & 0x7FFFFFFFFFFFFFFF      # 63 bits: bit 63 marks a device-resident seed

    def _check_mask(self, name: str, mask, B: int, n: int, device) -> None:
        """The checks of MultiheadAttention.forward's key_padding_mask; they need no device."""
        if not torch.is_tensor(mask) or mask.dtype not in (torch.bool, torch.uint8):
            raise ValueError(f"TransformerEncoder: {name} must be a torch.bool or torch.uint8 tensor (nonzero = padding)")
        if tuple(mask.shape) != (B, n):
            raise ValueError(f"TransformerEncoder: {name} of shape {tuple(mask.shape)}, expected [{B}, {n}]")
        if mask.device != device:
            raise ValueError(f"TransformerEncoder: {name} on {mask.device}, the inputs on {device}")

    def forward(self, x_in, x_in_k=None, x_in_v=None, *, encoder_padding_mask=None, key_padding_mask=None):
        self_form = x_in_k is None or x_in_v is None   # transformer.py:71,84: the self-attention stack
        if encoder_padding_mask is not None or key_padding_mask is not None:
            if x_in.dim() != 3:
                raise ValueError(f"TransformerEncoder: x_in of shape {tuple(x_in.shape)}, expected [T, B, {self.embed_dim}]")
            T, B = x_in.shape[0], x_in.shape[1]
            if key_padding_mask is not None:
                if self_form:
                    raise ValueError("TransformerEncoder: key_padding_mask marks the padding rows of x_in_k / x_in_v, and the "
                                     "self-attention call form has no key source; the padding rows of x_in are encoder_padding_mask")
                if x_in_k.dim() != 3:
                    raise ValueError(f"TransformerEncoder: x_in_k of shape {tuple(x_in_k.shape)}, expected [S, {B}, {self.embed_dim}]")
                self._check_mask("key_padding_mask", key_padding_mask, B, x_in_k.shape[0], x_in.device)
            if encoder_padding_mask is not None:
                if not self_form and not self.biprojection:
                    raise ValueError("TransformerEncoder: encoder_padding_mask hides padding rows of x_in as self-attention keys, "
                                     "and the crossmodal call of a plain (non-biprojection) encoder has no self-attention block "
                                     "that would read it; the padding rows of x_in_k / x_in_v are key_padding_mask")
                self._check_mask("encoder_padding_mask", encoder_padding_mask, B, T, x_in.device)
        self._ensure_store()
        if self_form:
            return _EncoderFn.apply(self._anchor, x_in, None, None, self, encoder_padding_mask, None)
        return _EncoderFn.apply(self._anchor, x_in, x_in_k, x_in_v, self, encoder_padding_mask, key_padding_mask)

    def attention_maps(self, layers=None, per_head: bool = False):
        """Head-averaged attention maps of the most recent forward call (either call form): a list with one entry per
        selected layer (None = all), each a dict from attention block to engine.AttentionMap(weights, query_steps) --
        {"cross": [B, T, S]} for the crossmodal call of a plain encoder, {"self": [B, T, T], "cross": [B, T, S]} for a
        biprojection one, {"self": [B, T, T]} for forward(x).  What a forward hook on layers[i].self_attn reads off the
        reference (the second return value of its MultiheadAttention, multihead_attention.py:132-135), with one stated
        difference: these are the softmax probabilities BEFORE attention dropout, equal to the reference's in eval mode
        and whenever attn_dropout == 0 (in training with dropout the reference returns the dropped, rescaled matrix).
        Detached fp32 tensors owned by the caller; nothing is computed for layers that are not selected, and nothing at
        all unless this is called.  Valid in train and eval mode, under no_grad or not, before or after backward(),
        until the next forward call; RuntimeError before the first one (or after .to() / .cuda() dropped the buffers).

        per_head=True: every head's probabilities instead of their mean, weights [B, H, T, S] (the [B * H, T, S] tensor the
        reference forms at multihead_attention.py:121, before it averages), same masks, same rules.  A map is then
        B * H * T * S * 4 bytes -- H times the averaged one, about 100 MB at B = 32, H = 3, T = S = 512: select `layers`."""
        if self._last_plan is None:
            raise RuntimeError("attention_maps: no forward pass to take the maps of (call forward first; .to() / .cuda() drop "
                               "the activation buffers)")
        return self._last_plan.attention_maps(None, layers, per_head)[0]
