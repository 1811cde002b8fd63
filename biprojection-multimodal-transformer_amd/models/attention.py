"""`MultiheadAttention` with the reference's constructor, call signature and state_dict layout
(bpmult/models/multihead_attention.py:17-135), executed on the HIP path.

forward(query, key, value, attn_mask, attn_bias, key_padding_mask) is one autograd node.  Its launches are those of the engine's self-attention
block (engine.py: _proj, _self_attn_fwd / _self_attn_bwd):

  forward   rows_cast            query / key / value -> CT rows (one problem per distinct input)
            gemm NT (grouped)    Q (alpha = dh^-0.5), K, V projections of in_proj_weight, OUT_HEADS epilogue
            attn_fwd[_amask | _kmask | _kamask]
                                 softmax(q k^T + attn_mask + attn_bias) v over the keys key_padding_mask leaves, dropout
                                 on the probabilities
            gemm NT              out_proj
            attn_maps[_amask | _kmask | _kamask]
                                 the head-averaged weights (need_weights only)
  backward  rows_cast            d(attn) -> CT, column sums = d(out_proj.bias)
            gemm TN / NN         d(out_proj.weight); d(attention output), OUT_HEADS
                                 (deterministic mode, the `deterministic` attribute: d(out_proj.bias) as this product's colsum_a)
            attn_bwd_dq / _dkv   [_amask | _kmask | _kamask]
            attn_bwd_dbias       d(attn_bias): the score gradient summed over samples (and heads), after the dQ pass;
                                 only when attn_bias requires grad (with the key masks beside a key_padding_mask)
            gemm TN (grouped)    the three row blocks of d(in_proj_weight), d(in_proj_bias) as colsum_a
            gemm NN (grouped)    d(query), d(key), d(value)

The parameters stay PyTorch's; their CT shadows are re-packed (bpm_pack_weights) when a version counter moves, the rule
of models/bert.py with text_params = "torch".  The effective additive image, attn_mask + attn_bias, is built by torch
copies (one add when both are given) in the layout the kernels read -- [Hm, T, ldm], rows padded to 4 columns, Hm = H for
a per-head bias and 1 otherwise, plus its transpose [Hm, S, ldt] for the dK / dV and maps kernels -- and kept until either
tensor's data_ptr or _version changes: a bias that an optimiser steps is copied again every forward (two copies of
Hm T S floats).  attn_mask gets no gradient; attn_bias gets one from bpm_attn_bwd_dbias, whose workspace lives in the
plan.  key_padding_mask ([B, S], nonzero = padding) becomes the kernels' visibility bytes (uint8 [B, S], nonzero = visible)
with one torch op (into a contiguous buffer: the mask may have any strides), kept until the tensor's data_ptr, _version or
shape changes -- a cache of its own: a padding mask
that changes every batch does not touch the additive image.  The family follows from what is given: neither -> the
unmasked entries, an image alone -> _amask, a padding mask alone -> _kmask, both -> _kamask.
attn_mask and attn_bias may also be per sample -- [Bm, Hm, T, S] with Bm in {1, B}, Hm in {1, H}, or torch's 3-D
[B*H, T, S] -- and attn_mask may be torch.bool (True hides); the one form attn_bias keeps refusing is the 4-D
[B, H, T, S] with B > 1 and H > 1, which is passed as [B*H, T, S].  effective_image() below builds their broadcast sum in the
smallest common form, [Bm, Hm, T, ldm] plus the transpose (2 Bm Hm T S 4 bytes); with Bm = B the same wrappers launch the
per-sample entries (_bmask / _kbmask, kernels of their own), and the bias gradient comes back in the bias's own shape
(bpm_attn_bwd_dbias_bmask: [B*H, T, S] is the score gradient itself, [B, 1, T, S] its sum over the heads of a sample).
add_bias_kv / add_zero_attn are refused.
"""
from __future__ import annotations

import weakref
from typing import Dict, Optional, Tuple

import torch
from torch import nn

from .. import config, ops
from .._lib import F_KPAD, GEMM_NN, GEMM_NT, GEMM_TN, OUT_HEADS, PackDesc
from ..ops import pad32

S_MHA_PROBS = 0x4d4841            # dropout site of the probabilities (any constant: the seed differs per call)


def _dhp_for(dh: int) -> int:
    for p in (32, 64, 128, 256):
        if dh <= p:
            return p
    raise ValueError(f"MultiheadAttention: head_dim {dh} > 256 has no HIP attention kernel")


_FORMS = "[T, S], [H, T, S], [Bm, Hm, T, S] with Bm in {1, B} and Hm in {1, H}, or torch's [B*H, T, S] (index b*H + h)"


def image_lead(shape, B: int, H: int, T: int, S: int, what: str = "attn_mask") -> Tuple[int, int]:
    """(Bm, Hm) of an additive image of `shape`, read as [Bm, Hm, T, S]: [T, S] -> (1, 1); [H, T, S] -> (1, H) (a 3-D
    tensor whose leading dimension is H keeps the per-head meaning; for B == 1 the two readings coincide); [B*H, T, S] ->
    (B, H); [Bm, Hm, T, S] as it stands -- except an attn_bias with Bm = B > 1 and Hm = H > 1, refused as before this
    function existed: it is passed as [B*H, T, S].  Any other shape: ValueError naming the accepted forms."""
    shape = tuple(shape)
    if shape[-2:] == (T, S):
        if len(shape) == 2:
            return 1, 1
        if len(shape) == 3 and shape[0] == H:
            return 1, H
        if len(shape) == 3 and shape[0] == B * H:
            return B, H
        if len(shape) == 4 and shape[0] in (1, B) and shape[1] in (1, H):
            # a 4-D attn_bias with B > 1 samples AND H > 1 heads stays refused, as it always was: that bias is spelled
            # [B*H, T, S] (bias.reshape(B * H, T, S), a view: the gradient flows through it)
            if what != "attn_bias" or shape[0] == 1 or shape[1] == 1:
                return shape[0], shape[1]
            raise ValueError(f"MultiheadAttention: attn_bias of shape {shape}; a bias per sample and head is passed in torch's 3-D "
                             f"form [B*H, T, S] = [{B * H}, {T}, {S}] (index b*H + h); the other forms are {_FORMS}")
    if what == "attn_mask":
        raise ValueError(f"MultiheadAttention: attn_mask must be a float or torch.bool tensor of shape {_FORMS} with B={B}, H={H}, "
                         f"T={T}, S={S}; got {shape}")
    raise ValueError(f"MultiheadAttention: {what} of shape {shape}; expected {_FORMS} with B={B}, H={H}, T={T}, S={S}")


def effective_image(attn_mask: Optional[torch.Tensor], attn_bias: Optional[torch.Tensor], B: int, H: int, T: int, S: int):
    """The image the kernels read for attn_mask + attn_bias, broadcast to the smallest common form (per sample if either
    argument is, per head if either is): (m, mt, ldm, ldt, head_stride, head_strideT, batch_stride, batch_strideT) with m
    fp32 [Bm, Hm, T, ldm], mt its transpose [Bm, Hm, S, ldt], leading dimensions rounded up to 4 (pad columns: zeros) and
    the strides in elements, 0 where the image is shared.  A torch.bool attn_mask hides where it is True (-inf / 0).  A
    pure function of its arguments on whatever device they live; it takes no part in autograd."""
    parts = []
    for t, what in ((attn_mask, "attn_mask"), (attn_bias, "attn_bias")):
        if t is None:
            continue
        bm, hm = image_lead(t.shape, B, H, T, S, what)
        t = t.detach()      # shares the storage (and the version counter), not the autograd graph of a non-leaf bias
        if t.dtype == torch.bool:
            t = torch.zeros(t.shape, device=t.device).masked_fill_(t, float("-inf"))
        parts.append(t.reshape(bm, hm, T, S).float())
    Bm, Hm = max(p.shape[0] for p in parts), max(p.shape[1] for p in parts)
    ldm, ldt = (S + 3) // 4 * 4, (T + 3) // 4 * 4
    m = torch.zeros(Bm, Hm, T, ldm, device=parts[0].device)
    mt = torch.zeros(Bm, Hm, S, ldt, device=parts[0].device)
    m[..., :S].copy_(parts[0].expand(Bm, Hm, T, S))
    if len(parts) == 2:
        m[..., :S].add_(parts[1])
    mt[..., :T].copy_(m[..., :S].transpose(2, 3))
    hs, hst = (T * ldm, S * ldt) if Hm > 1 else (0, 0)
    bs, bst = (Hm * T * ldm, Hm * S * ldt) if Bm > 1 else (0, 0)
    return m, mt, ldm, ldt, hs, hst, bs, bst


class _Plan:
    """Activation buffers of one (T, S, B, call form).  CT buffers are zero-initialised once: the launches write the
    embed_dim / head_dim columns only, the pad columns stay zero (the GEMMs read whole padded rows)."""

    def __init__(self, ex: "_Exec", T: int, S: int, B: int, form: str):
        self.T, self.S, self.B, self.form = T, S, B, form
        self.stamp = 0
        d, ld, H, dhp, dev = ex.d, ex.ld, ex.H, ex.dhp, ex.device
        ct = ops.ct_torch(ex.dtype)
        z = lambda *shape, dt=torch.float32: torch.zeros(*shape, device=dev, dtype=dt)
        self.xq = z(T * B, ld, dt=ct)
        self.xk = self.xq if form == "qkv" else z(S * B, ld, dt=ct)
        self.xv = self.xk if form in ("qkv", "kv") else z(S * B, ld, dt=ct)
        self.q, self.k, self.v = z(B, H, T, dhp, dt=ct), z(B, H, S, dhp, dt=ct), z(B, H, S, dhp, dt=ct)
        self.o, self.lse = z(T * B, ld, dt=ct), z(B, H, T)
        # backward
        self.dy, self.dao, self.delta = z(T * B, ld, dt=ct), z(B, H, T, dhp, dt=ct), z(B, H, T)
        self.dq, self.dk, self.dv = z(T * B, ld, dt=ct), z(S * B, ld, dt=ct), z(S * B, ld, dt=ct)
        self.mask = None             # (ops.attn_amasks array, the tensors it points into) of the forward pass; None: no attn_mask / attn_bias
        self.kmask = None            # (ops.attn_kmasks array, the bytes it points into) of the forward pass; None: no key_padding_mask
        self.dbias_ws = {}           # (samples, heads) of the bias gradient's form -> workspace of bpm_attn_bwd_dbias (None: no split)
        self.seed, self.drop_p = 0, 0.0


class _Exec:
    """Host driver of one module on one device and precision: CT weight shadows, plans, the mask cache."""

    def __init__(self, mod: "MultiheadAttention", device: torch.device, prec: str, det: bool = False):
        self.det = det       # deterministic mode: d(out_proj.bias) rides on the out_proj weight-gradient product (backward)
        if config.is_x3(prec):
            raise ValueError("MultiheadAttention: precision 'bf16x3' is not available for the stand-alone module (its split "
                             "images belong to an engine plan); use 'bf16' or 'f32'")
        self.device, self.prec, self.dtype = device, prec, config.dtype_code(prec)
        self.d, self.H, self.dh = mod.embed_dim, mod.num_heads, mod.head_dim
        self.ld, self.dhp, self.scale = pad32(self.d), _dhp_for(self.dh), mod.head_dim ** -0.5
        self.params = [p for p in (mod.in_proj_weight, mod.in_proj_bias, mod.out_proj.weight, mod.out_proj.bias) if p is not None]
        for p in self.params:
            if p.dtype != torch.float32 or not p.is_contiguous() or p.device != device:
                raise RuntimeError("MultiheadAttention: parameters must be contiguous float32 tensors on the inputs' device")
        self.key = (str(device), prec, tuple(p.data_ptr() for p in self.params), det)
        d, ld = self.d, self.ld
        ct = ops.ct_torch(self.dtype)
        self.shadow = torch.zeros(4 * d * ld, device=device, dtype=ct)        # in_proj_weight [3d, ld] | out_proj.weight [d, ld]
        descs, blk = [], 0
        for src, off, rows in ((mod.in_proj_weight, 0, 3 * d), (mod.out_proj.weight, 3 * d * ld, d)):
            pd = PackDesc()
            pd.src, pd.dst = src.data_ptr(), self.shadow.data_ptr() + self.shadow.element_size() * off
            pd.rows, pd.cols, pd.ld, pd.src_ld, pd.dst_ld, pd.blk0 = rows, d, ld, d, ld, blk
            pd.colscale = None
            blk += (rows * ld + 1023) // 1024
            descs.append(pd)
        self._pack = (ops.device_table(descs), len(descs), blk)
        self._versions = None
        self.plans: Dict[Tuple[int, int, int, str], _Plan] = {}
        self._mask_key, self._mask = None, None
        self._kmask_key, self._kmask, self._kmask_src = None, None, None

    def wptr(self, which: int) -> int:
        """Shadow of in_proj_weight rows [which d, (which + 1) d) (0 Q, 1 K, 2 V) or of out_proj.weight (3)."""
        return self.shadow.data_ptr() + self.shadow.element_size() * which * self.d * self.ld

    def refresh_shadows(self) -> None:
        sig = tuple(p._version for p in self.params)
        if sig != self._versions:
            ops.pack_weights(self.dtype, *self._pack)
            self._versions = sig

    def plan(self, T: int, S: int, B: int, form: str) -> _Plan:
        key = (T, S, B, form)
        pl = self.plans.get(key)
        if pl is None:
            pl = self.plans[key] = _Plan(self, T, S, B, form)
        return pl

    def mask_for(self, attn_mask: Optional[torch.Tensor], attn_bias: Optional[torch.Tensor], T: int, S: int, B: int):
        """The kernels' copy of the effective image attn_mask + attn_bias (effective_image: fp32 [Bm, Hm, T, ldm] and its
        transpose, Bm = B when either tensor is per sample, Hm = H when either is per head, else 1: stride 0); rebuilt when
        either tensor's storage or version counter, or the batch size, changes."""
        sig = lambda t: None if t is None else (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device))
        key = (sig(attn_mask), sig(attn_bias), B)
        if key != self._mask_key:
            m, mt, ldm, ldt, hs, hst, bs, bst = effective_image(attn_mask, attn_bias, B, self.H, T, S)
            # one image per sample: the 8-tuple form (the *_bmask / *_kbmask entries); otherwise the entries there always were
            desc = (m, ldm, mt, ldt, hs, hst) + ((bs, bst) if bs else ())
            # the source tensors are held too: while they live, their addresses cannot name other tensors
            srcs = [t.detach() for t in (attn_mask, attn_bias) if t is not None]
            self._mask = (ops.attn_amasks([desc]), m, mt, srcs)
            self._mask_key = key
        return self._mask

    def kmask_for(self, key_padding_mask: torch.Tensor):
        """The kernels' copy of key_padding_mask: uint8 [B, S], nonzero where the key is VISIBLE (the *_kmask convention, the
        opposite of the argument's); rebuilt when the tensor's storage, version counter or shape changes."""
        t = key_padding_mask
        key = (t.data_ptr(), t._version, tuple(t.shape), tuple(t.stride()), t.dtype, str(t.device))
        # the key holds for the tensor it was taken from only (a weak reference: the caller's mask is not kept alive, and
        # once it is gone its address may name another tensor)
        if key != self._kmask_key or self._kmask_src() is not t:
            vis = torch.empty(t.shape, dtype=torch.bool, device=t.device)     # contiguous [B, S] whatever t's strides are
            torch.eq(t, 0, out=vis)                                           # the one kernel
            vis = vis.view(torch.uint8)                                       # renames bool's 0 / 1 bytes
            self._kmask = (ops.attn_kmasks([(vis, t.shape[1])]), vis)
            self._kmask_key, self._kmask_src = key, weakref.ref(t)
        return self._kmask

    # -- the four families: no mask, additive image, key bytes, both ----------------------------------------------------
    @staticmethod
    def _attn(pl: "_Plan", which: str, dt: int, probs, seed: int) -> None:
        """which: 'fwd', 'bwd_dq' or 'bwd_dkv', through the entry of the plan's masks."""
        if pl.mask is None and pl.kmask is None:
            getattr(ops, f"attn_{which}")(dt, probs, seed)
        elif pl.kmask is None:
            getattr(ops, f"attn_{which}_amask")(dt, probs, pl.mask[0], seed)
        elif pl.mask is None:
            getattr(ops, f"attn_{which}_kmask")(dt, probs, pl.kmask[0], seed)
        else:
            getattr(ops, f"attn_{which}_kamask")(dt, probs, pl.kmask[0], pl.mask[0], seed)

    # -- forward -------------------------------------------------------------------------------------------------------
    def forward(self, mod, query, key, value, form, attn_mask, attn_bias, need_weights, seed, training, key_padding_mask=None):
        T, B, d = query.shape
        S = key.shape[0]
        self.refresh_shadows()
        pl = self.plan(T, S, B, form)
        pl.stamp += 1
        dt, ld, H, dh, dhp = self.dtype, self.ld, self.H, self.dh, self.dhp
        pl.mask = None if attn_mask is None and attn_bias is None else self.mask_for(attn_mask, attn_bias, T, S, B)
        pl.kmask = None if key_padding_mask is None else self.kmask_for(key_padding_mask)
        pl.seed, pl.drop_p = seed, (mod.attn_dropout if training else 0.0)
        casts = [ops.cast_problem(query, d, T * B, d, dst_ct=pl.xq, ldd=ld)]
        if form != "qkv":
            casts.append(ops.cast_problem(key, d, S * B, d, dst_ct=pl.xk, ldd=ld))
        if form == "sep":
            casts.append(ops.cast_problem(value, d, S * B, d, dst_ct=pl.xv, ldd=ld))
        ops.rows_cast(dt, casts, 0)
        bias = mod.in_proj_bias
        proj = [ops.gemm_problem(x, self.wptr(w), out, L * B, d, d, ld, ld, 0, bias_n=None if bias is None else bias[w * d:(w + 1) * d],
                                 alpha=self.scale if w == 0 else 1.0, out_kind=OUT_HEADS, heads=(B, H, L, dh, dhp), flags=F_KPAD)
                for w, (x, out, L) in enumerate(((pl.xq, pl.q, T), (pl.xk, pl.k, S), (pl.xv, pl.v, S)))]
        ops.gemm_grouped(dt, GEMM_NT, proj, seed)
        ap = [ops.attn_problem(pl.q, pl.k, pl.v, pl.o, ld, pl.lse, B, H, T, S, dh, dhp, 0, drop_p=pl.drop_p, drop_site=S_MHA_PROBS)]
        self._attn(pl, "fwd", dt, ap, seed)
        out = torch.empty(T, B, d, device=self.device)
        ops.gemm_grouped(dt, GEMM_NT, [ops.gemm_problem(pl.o, self.wptr(3), out, T * B, d, d, ld, ld, d, bias_n=mod.out_proj.bias,
                                                        flags=F_KPAD)], seed)
        weights = None
        if need_weights:
            # need_weights == "heads" (average_attn_weights=False): one map per head, through the bpm_attn_head_maps family
            heads = need_weights == "heads"
            weights = torch.empty((B, H, T, S) if heads else (B, T, S), device=self.device)
            mp = [(ops.attn_head_map_problem if heads else ops.attn_map_problem)(pl.q, pl.k, pl.lse, weights, S, B, H, T, S, dh, dhp, 0)]
            maps = "attn_head_maps" if heads else "attn_maps"
            if pl.mask is None and pl.kmask is None:
                getattr(ops, maps)(dt, mp)
            elif pl.kmask is None:
                getattr(ops, maps + "_amask")(dt, mp, pl.mask[0])
            elif pl.mask is None:
                getattr(ops, maps + "_kmask")(dt, mp, pl.kmask[0])
            else:
                getattr(ops, maps + "_kamask")(dt, mp, pl.kmask[0], pl.mask[0])
        return out, weights, pl

    # -- backward ------------------------------------------------------------------------------------------------------
    def backward(self, mod, pl: _Plan, dout: torch.Tensor, bias_shape=None):
        """dout fp32 [T, B, d] -> d(query), d(key), d(value), d(attn_bias) (None unless bias_shape, the shape of the bias
        that wants one, is given) and the parameter gradients in self.params order: fresh tensors every call (autograd
        may keep them as .grad)."""
        T, S, B = pl.T, pl.S, pl.B
        dt, d, ld, H, dh, dhp, seed, dev = self.dtype, self.d, self.ld, self.H, self.dh, self.dhp, pl.seed, self.device
        has_bias = mod.in_proj_bias is not None
        g_ipw, g_wo = torch.empty(3 * d, d, device=dev), torch.empty(d, d, device=dev)       # written by their launches
        g_ipb = torch.zeros(3 * d, device=dev) if has_bias else None                           # accumulated into: zeroed
        g_ob = torch.zeros(d, device=dev) if mod.out_proj.bias is not None else None
        # d(out_proj.bias): the column sums of dout by the cast launch (float atomics), or -- deterministic mode -- of dy as
        # stored, by the weight-gradient product that reads it (colsum_a: one owner per column, k ascending)
        ops.rows_cast(dt, [ops.cast_problem(dout, d, T * B, d, dst_ct=pl.dy, ldd=ld, colsum=None if self.det else g_ob)], 0)
        ops.gemm_grouped(dt, GEMM_TN, [ops.gemm_problem(pl.dy, pl.o, g_wo, d, d, T * B, ld, ld, d, flags=F_KPAD,
                                                        colsum_a=g_ob if self.det else None)], seed)
        ops.gemm_grouped(dt, GEMM_NN, [ops.gemm_problem(pl.dy, self.wptr(3), pl.dao, T * B, d, d, ld, ld, 0, out_kind=OUT_HEADS,
                                                        heads=(B, H, T, dh, dhp), flags=F_KPAD)], seed)
        ap = [ops.attn_problem(pl.q, pl.k, pl.v, pl.o, ld, pl.lse, B, H, T, S, dh, dhp, 0, dO=pl.dao, delta=pl.delta, dQ=pl.dq, lddq=ld,
                               dK=pl.dk, lddk=ld, dV=pl.dv, lddv=ld, dq_scale=self.scale, drop_p=pl.drop_p, drop_site=S_MHA_PROBS)]
        self._attn(pl, "bwd_dq", dt, ap, seed)
        self._attn(pl, "bwd_dkv", dt, ap, seed)
        g_bias = None
        if bias_shape is not None:
            g_bias = self.bias_grad(pl, ap, bias_shape, seed)
        sides = ((pl.dq, pl.xq, T), (pl.dk, pl.xk, S), (pl.dv, pl.xv, S))
        ops.gemm_grouped(dt, GEMM_TN, [ops.gemm_problem(g, x, g_ipw.data_ptr() + 4 * w * d * d, d, d, L * B, ld, ld, d, flags=F_KPAD,
                                                        colsum_a=g_ipb.data_ptr() + 4 * w * d if has_bias else None)
                                       for w, (g, x, L) in enumerate(sides)], seed)
        dx = [torch.empty(L, B, d, device=dev) for L in (T, S, S)]
        ops.gemm_grouped(dt, GEMM_NN, [ops.gemm_problem(g, self.wptr(w), dx[w], L * B, d, d, ld, ld, d, flags=F_KPAD)
                                       for w, (g, _, L) in enumerate(sides)], seed)
        grads = [g for g in (g_ipw, g_ipb, g_wo, g_ob) if g is not None]
        return dx[0], dx[1], dx[2], g_bias, grads

    def bias_grad(self, pl: _Plan, ap, bias_shape, seed: int) -> torch.Tensor:
        """d(attn_bias) of the plan's last forward pass, after its dQ pass has left delta: fp32, bias_shape ([T, S]: summed
        over samples and heads; [H, T, S]: over samples); a pair the effective image hides gets exactly 0, and a sample
        adds nothing at the keys its key_padding_mask hides."""
        T, S = pl.T, pl.S
        # the form of the result follows from the bias alone: one image per sample and / or head that the bias has its own
        Bb, Hb = image_lead(bias_shape, pl.B, self.H, T, S, "attn_bias")
        nimg = (Bb, Hb)
        ldb = (S + 3) // 4 * 4
        g = torch.empty(Bb, Hb, T, ldb, device=self.device)
        hs = T * ldb if Hb > 1 else 0
        # a per-sample result goes through bpm_attn_bwd_dbias_bmask (the 4-tuple form), as does any result under per-sample masks
        outs = ops.attn_dbias([(g, ldb, hs, Hb * T * ldb) if Bb > 1 else (g, ldb, hs)])
        if nimg not in pl.dbias_ws:
            n = ops.attn_dbias_ws_bytes(ap, outs)
            pl.dbias_ws[nimg] = torch.empty((n + 3) // 4, device=self.device) if n else None
        if pl.kmask is None:
            ops.attn_bwd_dbias(self.dtype, ap, pl.mask[0], outs, seed, ws=pl.dbias_ws[nimg])
        else:
            ops.attn_bwd_dbias(self.dtype, ap, pl.mask[0], outs, seed, ws=pl.dbias_ws[nimg], kmasks=pl.kmask[0])
        g = g if ldb == S else g[..., :S].contiguous()
        return g.reshape(bias_shape)

class _MhaFn(torch.autograd.Function):
    """The whole call as one autograd node: (query, key, value, attn_bias, parameters) -> (attn, head-averaged weights or
    None)."""

    @staticmethod
    def forward(ctx, query, key, value, mod, ex, form, attn_mask, need_weights, seed, attn_bias, key_padding_mask, *params):
        out, weights, plan = ex.forward(mod, query.detach().contiguous(), key.detach().contiguous(), value.detach().contiguous(), form,
                                        attn_mask, attn_bias, need_weights, seed, mod.training, key_padding_mask)
        ctx.mod, ctx.ex, ctx.plan, ctx.stamp = mod, ex, plan, plan.stamp
        ctx.bias_shape = None if attn_bias is None else tuple(attn_bias.shape)
        if weights is None:
            return out, None
        ctx.mark_non_differentiable(weights)
        return out, weights

    @staticmethod
    def backward(ctx, dout, _dweights=None):
        if ctx.stamp != ctx.plan.stamp:
            raise RuntimeError("MultiheadAttention (HIP path): backward() of a forward pass that a later forward pass of the same "
                               "shape has overwritten; run forward -> backward one call at a time")
        need = ctx.needs_input_grad
        dq, dk, dv, g_bias, grads = ctx.ex.backward(ctx.mod, ctx.plan, dout.contiguous().float(), ctx.bias_shape if need[9] else None)
        return ((dq if need[0] else None, dk if need[1] else None, dv if need[2] else None, None, None, None, None, None, None, g_bias, None)
                + tuple(g if n else None for g, n in zip(grads, need[11:])))


class MultiheadAttention(nn.Module):
    """Drop-in for bpmult.models.multihead_attention.MultiheadAttention (packed in-projection, :17-50).

    forward(query, key, value, attn_mask=None, need_weights=True, attn_bias=None, key_padding_mask=None,
    average_attn_weights=True) -> (attn [T, B, d], weights [B, T, S] ([B, H, T, S] with average_attn_weights=False) or None) on
    [T,B,d] / [S,B,d] fp32 CUDA (HIP) tensors, in the reference's three call forms (query is key is value; key is value;
    three tensors).  attn_mask: None or a float [T, S] tensor added to the scores of every head (-inf hides a pair; every
    row must keep a visible key, or it is NaN as in the reference); it gets no gradient (requires_grad: ValueError).
    attn_bias (an extension): None or a float32 tensor on the inputs' device, [T, S] (added to the scores of every head) or
    [H, T, S] (head h of every sample gets attn_bias[h]), finite or -inf entries; the scores get attn_mask + attn_bias.  It
    may require grad -- an nn.Parameter, or a non-leaf such as a gather from a relative-position table: its gradient (the
    score gradient summed over samples, and over heads for [T, S]; exactly 0 where the effective entry is -inf) comes back
    through autograd.  `weights` are taken under the same mask + bias.
    Per-sample forms (attn_mask and attn_bias alike): [Bm, Hm, T, S] with Bm in {1, B} and Hm in {1, H}, and
    torch.nn.MultiheadAttention's 3-D [B*H, T, S], read as [B, H, T, S] (index b*H + h); a 3-D tensor whose leading dimension
    is H keeps the per-head meaning (for B = 1 the two readings coincide).  attn_mask may also be torch.bool in any of these
    shapes, True hiding the pair (torch's convention).  The scores get the broadcast sum, per sample if either argument is
    and per head if either is; the kernels' copy of it and of its transpose costs 2 * Bm * Hm * T * S * 4 bytes.  The
    gradient of attn_bias comes back in the bias's own shape -- [B*H, T, S]: the score gradient; [B, 1, T, S]: summed over
    the heads of the sample -- whatever the form of the mask beside it.  One spelling stays refused for attn_bias, as it
    always was: the 4-D [B, H, T, S] with B > 1 and H > 1 (pass bias.reshape(B * H, T, S), a view).  Any other shape: ValueError naming these forms.
    key_padding_mask (the reference's docstring, :56-58): None or a torch.bool / torch.uint8 tensor [B, S] on the inputs'
    device; nonzero / True marks padding: that key is hidden for every head and query of its sample -- probability and
    `weights` exactly 0, d(key) / d(value) rows of a padded position exactly 0 -- alone or beside attn_mask / attn_bias.
    Query rows are never masked; every query row of every sample must keep a visible key under all masks together (not
    checked; NaN otherwise).  It gets no gradient.
    One stated difference: `weights` are the head-averaged softmax probabilities BEFORE attention dropout, detached --
    equal to the reference's in eval mode and whenever attn_dropout == 0 (in training with dropout the reference returns
    the dropped, rescaled matrix); the departure TransformerEncoder.attention_maps() makes.  need_weights=False (an
    extension) launches nothing for them and returns None.  average_attn_weights=False (torch's name for the switch): the
    probabilities of every head, [B, H, T, S] -- the tensor the reference averages (:121) -- under the same attn_mask,
    attn_bias and key_padding_mask, before dropout, detached and non-differentiable like the averaged one; H times its
    size (B * H * T * S * 4 bytes).  add_bias_kv / add_zero_attn are not supported (ValueError).
    Precision: the `precision` attribute, or config.precision() when it is None ('bf16' or 'f32').
    TransformerEncoder constructs this class as a parameter container and runs its own grouped engine plan."""

    def __init__(self, embed_dim: int, num_heads: int, attn_dropout: float = 0.0, bias: bool = True, add_bias_kv: bool = False,
                 add_zero_attn: bool = False):
        super().__init__()
        if add_bias_kv or add_zero_attn:
            raise ValueError("MultiheadAttention: add_bias_kv / add_zero_attn are not supported on the HIP path")
        self.embed_dim, self.num_heads, self.attn_dropout = embed_dim, num_heads, attn_dropout
        self.head_dim = embed_dim // num_heads
        if self.head_dim * num_heads != embed_dim:
            raise ValueError("embed_dim must be divisible by num_heads")
        self.scaling = self.head_dim ** -0.5
        self.in_proj_weight = nn.Parameter(torch.empty(3 * embed_dim, embed_dim))
        if bias:
            self.in_proj_bias = nn.Parameter(torch.zeros(3 * embed_dim))
        else:
            self.register_parameter("in_proj_bias", None)
        self.out_proj = nn.Linear(embed_dim, embed_dim, bias=bias)
        self.bias_k = self.bias_v = None
        self.add_zero_attn = False
        nn.init.xavier_uniform_(self.in_proj_weight)          # fan computed on the packed shape (:41-46)
        nn.init.xavier_uniform_(self.out_proj.weight)
        if bias:
            nn.init.constant_(self.out_proj.bias, 0.0)
        self.precision: Optional[str] = None                  # None -> config.precision() at first use
        self.deterministic: Optional[bool] = None             # None -> config.deterministic(), read when the driver is built
        self._exec: Optional[_Exec] = None
        self._step = 0

    def _apply(self, fn, *a, **k):
        r = super()._apply(fn, *a, **k)
        self._exec = None                                     # .to() / .cuda(): plans, shadows and the mask copy go
        return r

    def invalidate_shadows(self) -> None:
        """The next forward re-packs the CT weight shadows whatever the version counters say (after a write through
        `p.data`, which moves none)."""
        if self._exec is not None:
            self._exec._versions = None

    def _next_seed(self) -> int:                              # the formula of TransformerEncoder._next_seed
        self._step += 1
        return (torch.initial_seed() * 1000003 + self._step) & 0x7FFFFFFFFFFFFFFF

    def _ensure_exec(self, device: torch.device) -> _Exec:
        prec = self.precision or config.precision()
        ex = self._exec
        params = [p for p in (self.in_proj_weight, self.in_proj_bias, self.out_proj.weight, self.out_proj.bias) if p is not None]
        det = config.resolve_deterministic(self.deterministic)
        if ex is None or ex.key != (str(device), prec, tuple(p.data_ptr() for p in params), det):
            ex = self._exec = _Exec(self, device, prec, det)
        return ex

    def forward(self, query, key, value, attn_mask=None, need_weights: bool = True, attn_bias=None, key_padding_mask=None,
                average_attn_weights: bool = True):
        if query.dim() != 3 or query.shape[2] != self.embed_dim:
            raise ValueError(f"MultiheadAttention: query of shape {tuple(query.shape)}, expected [T, B, {self.embed_dim}]")
        T, B, d = query.shape
        if key.shape != value.shape or key.dim() != 3 or key.shape[1:] != (B, d):
            raise ValueError(f"MultiheadAttention: key {tuple(key.shape)} / value {tuple(value.shape)}, expected two [S, {B}, {d}] tensors")
        for t in (query, key, value):
            if t.dtype != torch.float32:
                raise ValueError(f"MultiheadAttention: expected float32 inputs, got {t.dtype}")
        S = key.shape[0]
        same = lambda a, b: a is b or (a.data_ptr() == b.data_ptr() and a.shape == b.shape and a.stride() == b.stride())
        form = "qkv" if same(query, key) and same(key, value) else "kv" if same(key, value) else "sep"
        if attn_mask is not None:
            if not torch.is_tensor(attn_mask) or not (attn_mask.is_floating_point() or attn_mask.dtype == torch.bool):
                raise ValueError(f"MultiheadAttention: attn_mask must be a float or torch.bool tensor of shape {_FORMS}")
            image_lead(attn_mask.shape, B, self.num_heads, T, S, "attn_mask")
            if attn_mask.requires_grad:
                raise ValueError("MultiheadAttention: attn_mask gets no gradient on the HIP path (requires_grad is set)")
        if attn_bias is not None:
            if not torch.is_tensor(attn_bias) or attn_bias.dtype != torch.float32:
                raise ValueError("MultiheadAttention: attn_bias must be a float32 tensor")
            image_lead(attn_bias.shape, B, self.num_heads, T, S, "attn_bias")
            if attn_bias.device != query.device:
                raise ValueError(f"MultiheadAttention: attn_bias on {attn_bias.device}, the inputs on {query.device}")
            if config.is_x3(self.precision or config.precision()):
                raise ValueError("MultiheadAttention: attn_bias is not available with precision 'bf16x3'; use 'bf16' or 'f32'")
        if key_padding_mask is not None:
            if not torch.is_tensor(key_padding_mask) or key_padding_mask.dtype not in (torch.bool, torch.uint8):
                raise ValueError("MultiheadAttention: key_padding_mask must be a torch.bool or torch.uint8 tensor (nonzero = padding)")
            if tuple(key_padding_mask.shape) != (B, S):
                raise ValueError(f"MultiheadAttention: key_padding_mask of shape {tuple(key_padding_mask.shape)}, expected [{B}, {S}]")
            if key_padding_mask.device != query.device:
                raise ValueError(f"MultiheadAttention: key_padding_mask on {key_padding_mask.device}, the inputs on {query.device}")
            if config.is_x3(self.precision or config.precision()):
                raise ValueError("MultiheadAttention: key_padding_mask is not available with precision 'bf16x3'; use 'bf16' or 'f32'")
        for t in (query, key, value):             # after the argument checks: those need no device
            if not t.is_cuda:
                raise RuntimeError("MultiheadAttention: the HIP attention path needs CUDA (HIP) tensors; there is no CPU path")
        ex = self._ensure_exec(query.device)
        seed = self._next_seed()
        want = False if not need_weights else True if average_attn_weights else "heads"
        return _MhaFn.apply(query, key, value, self, ex, form, attn_mask, want, seed, attn_bias, key_padding_mask, *ex.params)
