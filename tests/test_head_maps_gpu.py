"""Per-head attention maps on the MI355X (bpm_attn_head_maps and its four masked siblings, attention_maps(per_head=True),
MultiheadAttention(average_attn_weights=False)).

1. The kernel through the C ABI against float64 torch from the same rounded Q / K (softmax in float64), LSE taken from
   bpm_attn_fwd* on the same inputs.  Limit: tests/test_attn_maps_gpu.py's `tol()` (f32 2e-5, bf16 1.5e-2): a per-head
   value is one addend of what that test bounds, from the same arithmetic, and probabilities are <= 1.  Hidden pairs
   compare == 0, rows sum to 1 within the limit, pad columns and the gaps between heads and samples keep a sentinel.
2. Per head, not merely on average: P_h . V in float64 from the kernel's maps reproduces the O that bpm_attn_fwd wrote,
   head by head, under the limit and comparison tests/test_kernels_gpu.py applies to the forward output (3e-5 / 2e-2 of
   max(1, |O|max)).  A head permutation or a wrong head offset passes a head-mean check and fails this one.
3. Against the averaged kernel on the same buffers, all five families: the fp32 sum over h ascending times 1/H within 2e-5
   in both dtypes (both kernels read the same Q / K / LSE: only fp32 arithmetic separates them).  Prints whether the two
   are bit-equal.
4. Masks at T 65, S 129 (the mask shape of tests/attn_cases.py); two calls give identical bits.
5. The reference's per-head probabilities (fixture head_maps.npz, tests/golden/make_golden_head_maps.py) through
   TransformerEncoder, the 3-modal model (both schedules, eager and graph replay) and MultiheadAttention.  f32: 2e-4, the
   limit tests/test_attn_maps_gpu.py uses on the same cases.  bf16 / bf16x3: max-abs and relative-L2 error per case, <= 2x
   the errors measured on the MI355X (MEASURED below; profiles/head_maps_errors.json, written through BPMULT_ERROR_LOG).
6. Properties: taking per-head maps changes neither the following backward() nor the next step's bits; per_head=False
   after per_head=True returns the same bits as before; shapes and query_steps under the pruned schedule."""
import copy
import json
import os
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from detgen import det, det_param  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import ops  # noqa: E402
from bpmult_amd._lib import BPM_BF16, BPM_F32  # noqa: E402
from bpmult_amd.engine import dhp_for  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.models.attention import MultiheadAttention  # noqa: E402
from bpmult_amd.models.encoder import TransformerEncoder  # noqa: E402

import mha_kpm_cases  # noqa: E402

G = os.path.join(os.path.dirname(__file__), "golden")
T = torch.from_numpy
DEV = "cuda"
B = 2
SENTINEL = 7.0
NINF = float("-inf")


def tol(dtype):                      # == tests/test_attn_maps_gpu.py:tol == tests/test_kernels_gpu.py:tol
    return 2e-5 if dtype == BPM_F32 else 1.5e-2


def tol_o(dtype):                    # tests/test_kernels_gpu.py: the forward output against float64, times max(1, |ref|max)
    return 3e-5 if dtype == BPM_F32 else 2e-2


SUM_LIMIT = 2e-5                     # head sum against the averaged kernel, both dtypes


def rnd(*shape, seed=0, scale=1.0):
    g = torch.Generator().manual_seed(seed)
    return torch.randn(*shape, generator=g) * scale


# ---------------------------------------------------------------------------------------------------------------------
# 1.-4. kernel
# ---------------------------------------------------------------------------------------------------------------------
class Problem:
    """Random Q / K / V in the head-major padded layout, O and LSE by the forward entry of the masks' family, the float64
    probabilities [B, H, T, S] from the same rounded operands, and a sentinel-filled output with a gap after every head
    and every sample."""

    def __init__(self, dtype, Bn, H, Tn, S, dh, masked=True, qpos=None, kvis=None, add=None, seed=0):
        self.dtype, self.dims = dtype, (Bn, H, Tn, S, dh)
        dhp, ctt = dhp_for(dh), ops.ct_torch(dtype)
        self.dhp, self.ld = dhp, ops.pad32(H * dh)

        def heads(x):
            buf = torch.zeros(*x.shape[:3], dhp, dtype=ctt)
            buf[..., :dh] = x.to(ctt)
            return buf.to(DEV), buf[..., :dh].double()

        self.Q, q = heads(rnd(Bn, H, Tn, dh, seed=31 + seed) * dh ** -0.5 * 2.0)
        self.K, k = heads(rnd(Bn, H, S, dh, seed=32 + seed) * 1.5)
        self.V, self.v = heads(rnd(Bn, H, S, dh, seed=33 + seed))
        p0, st = qpos if qpos is not None else (0, 1)
        self.qpos = (p0, st)
        Tfull = p0 + (Tn - 1) * st + 1
        self.off = 1 + abs(S - Tfull) if masked else 0
        self.O = torch.zeros(Tn * Bn, self.ld, device=DEV, dtype=ctt)
        self.lse = torch.zeros(Bn, H, Tn, device=DEV)
        # masks as the entries take them
        self.kmasks = self.amasks = None
        self.keep = []
        if kvis is not None:                        # bool [B, S], True = visible
            vis = kvis.to(torch.uint8).to(DEV)
            self.kmasks = ops.attn_kmasks([(vis, S)])
            self.keep.append(vis)
        if add is not None:                         # fp32 [T, S] or [H, T, S]
            a3 = add if add.dim() == 3 else add[None]
            Hm = a3.shape[0]
            ldm, ldt = (S + 3) // 4 * 4, (Tn + 3) // 4 * 4
            m, mt = torch.zeros(Hm, Tn, ldm), torch.zeros(Hm, S, ldt)
            m[:, :, :S] = a3
            mt[:, :, :Tn] = a3.transpose(1, 2)
            m, mt = m.to(DEV), mt.to(DEV)
            self.amasks = ops.attn_amasks([(m, ldm, mt, ldt) + ((Tn * ldm, S * ldt) if Hm > 1 else (0, 0))])
            self.keep += [m, mt]
        ap = [ops.attn_problem(self.Q, self.K, self.V, self.O, self.ld, self.lse, Bn, H, Tn, S, dh, dhp, self.off, q_pos0=p0, q_stride=st)]
        self.call(("attn_fwd",), ap)
        # float64 reference
        s = q @ k.transpose(-1, -2)
        hidden = torch.zeros(Bn, H, Tn, S, dtype=torch.bool)
        if masked:
            i = p0 + st * torch.arange(Tn)[:, None]
            hidden |= ((torch.arange(S)[None, :] - i) >= self.off)[None, None]
        if kvis is not None:
            hidden |= ~kvis[:, None, None, :]
        if add is not None:
            a3 = (add if add.dim() == 3 else add[None]).double()
            s = s + a3[None]
            hidden |= torch.isinf(a3)[None].expand(Bn, -1, -1, -1) if a3.shape[0] == H else torch.isinf(a3)[None].expand(Bn, H, -1, -1)
        self.hidden = hidden
        self.ref = torch.softmax(s.masked_fill(hidden, NINF), -1)

    def call(self, names, probs, *more):
        """ops.<name>[_kmask | _amask | _kamask] of this problem's masks; names: (base,) or (base, name for per-head images)"""
        base = names[0]
        if self.kmasks is None and self.amasks is None:
            getattr(ops, base)(self.dtype, probs, *more)
        elif self.amasks is None:
            getattr(ops, base + "_kmask")(self.dtype, probs, self.kmasks, *more)
        elif self.kmasks is None:
            getattr(ops, base + names[-1] if len(names) > 1 else base + "_amask")(self.dtype, probs, self.amasks, *more)
        else:
            getattr(ops, base + "_kamask")(self.dtype, probs, self.kmasks, self.amasks, *more)

    def output(self, ldw=None, gap=True):
        Bn, H, Tn, S, dh = self.dims
        self.ldw = S if ldw is None else ldw
        self.hs = Tn * self.ldw + (12 if gap else 0)
        self.bs = H * self.hs + (20 if gap else 0)
        self.flat = torch.full((Bn * self.bs,), SENTINEL, device=DEV)
        return ops.attn_head_map_problem(self.Q, self.K, self.lse, self.flat, self.ldw, Bn, H, Tn, S, dh, self.dhp, self.off,
                                         q_pos0=self.qpos[0], q_stride=self.qpos[1], head_stride=self.hs, batch_stride=self.bs)

    def maps(self):
        Bn, H, Tn, S, dh = self.dims
        return self.flat.as_strided((Bn, H, Tn, S), (self.bs, self.hs, self.ldw, 1))

    def averaged(self):
        """The averaged entry of the same family on the same buffers -> [B, T, S]"""
        Bn, H, Tn, S, dh = self.dims
        W = torch.full((Bn, Tn, S), SENTINEL, device=DEV)
        mp = [ops.attn_map_problem(self.Q, self.K, self.lse, W, S, Bn, H, Tn, S, dh, self.dhp, self.off, q_pos0=self.qpos[0], q_stride=self.qpos[1])]
        self.call(("attn_maps",), mp)
        return W

    def check(self, what):
        Bn, H, Tn, S, dh = self.dims
        dtype = self.dtype
        torch.cuda.synchronize()
        P = self.maps()
        got = P.double().cpu()
        assert torch.isfinite(got).all(), what
        # only W[b][h][i][0 .. S) is written
        written = torch.zeros_like(self.flat, dtype=torch.bool)
        written.as_strided((Bn, H, Tn, S), (self.bs, self.hs, self.ldw, 1)).fill_(True)
        assert int(written.sum()) == Bn * H * Tn * S
        assert (self.flat[~written] == SENTINEL).all(), what + ": a pad column or a gap between heads / samples was written"
        err = (got - self.ref).abs().max().item()
        rows = (got.sum(-1) - 1.0).abs().max().item()
        print(f"{what}: max err {err:.3e}, row sums off by {rows:.3e} (limit {tol(dtype):.1e})")
        assert (got[self.hidden] == 0).all(), what + ": hidden pairs must be exactly 0"
        assert err <= tol(dtype), f"{what}: max err {err:.3e} > {tol(dtype):.1e}"
        assert rows <= tol(dtype), f"{what}: row sums off by {rows:.3e} > {tol(dtype):.1e}"
        # per head: P_h . V reproduces the forward's O (drop_p = 0)
        d = H * dh
        o = self.O[:, :d].float().reshape(Tn, Bn, H, dh).permute(1, 2, 0, 3).double().cpu()
        pv = got @ self.v
        scale = max(1.0, o.abs().max().item())
        eo = (pv - o).abs().amax(dim=(0, 2, 3))
        print(f"{what}: |P_h V - O_h| per head {[f'{e:.2e}' for e in eo.tolist()]} (limit {tol_o(dtype) * scale:.2e})")
        assert (eo <= tol_o(dtype) * scale).all(), f"{what}: P_h V does not reproduce O head by head: {eo.tolist()}"
        # the averaged kernel on the same buffers: sum over h ascending in fp32, times 1/H
        avg = self.averaged()
        acc = torch.zeros(Bn, Tn, S, device=DEV)
        for h in range(H):
            acc += P[:, h]
        acc *= (torch.ones((), device=DEV) / torch.full((), float(H), device=DEV))
        es = (acc - avg).abs().max().item()
        print(f"{what}: head sum against the averaged kernel: max diff {es:.3e}, bit-equal: {torch.equal(acc, avg)}")
        assert es <= SUM_LIMIT, f"{what}: head sum differs from the averaged kernel by {es:.3e} > {SUM_LIMIT:.1e}"


# (B, H, T, S, dh, masked, (q_pos0, q_stride))
KERNEL_SHAPES = [(2, 3, 70, 100, 25, True, None), (2, 2, 100, 70, 6, True, None), (1, 1, 33, 65, 64, False, None),
                 (1, 2, 130, 130, 64, True, None), (1, 2, 2, 200, 25, True, (0, 199)), (1, 6, 50, 50, 128, True, None),
                 (1, 2, 70, 130, 256, True, None), (1, 1, 1, 1, 25, True, None)]
DTYPES = pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16], ids=["f32", "bf16"])


@DTYPES
@pytest.mark.parametrize("Bn,H,Tn,S,dh,masked,qpos", KERNEL_SHAPES)
def test_kernel_against_float64(dtype, Bn, H, Tn, S, dh, masked, qpos):
    pr = Problem(dtype, Bn, H, Tn, S, dh, masked, qpos)
    ops.attn_head_maps(dtype, [pr.output(ldw=S + 5 if S % 2 else None)])
    pr.check(f"{Bn}x{H}x{Tn}x{S} dh {dh}")


@DTYPES
def test_kernel_three_problems_of_mixed_sizes(dtype):
    shapes = [(2, 3, 70, 100, True, None, 104), (1, 2, 130, 64, True, None, 64), (2, 2, 2, 96, True, (0, 95), 101)]
    made = [Problem(dtype, Bn, H, Tn, S, 25, m, qp, seed=7 * n) for n, (Bn, H, Tn, S, m, qp, _) in enumerate(shapes)]
    ops.attn_head_maps(dtype, [pr.output(ldw=sh[-1]) for pr, sh in zip(made, shapes)])
    for n, (pr, sh) in enumerate(zip(made, shapes)):
        pr.check(f"problem {n} {sh}")


# masks at the mask shape of tests/attn_cases.py
MT, MS, MH = 65, 129, 3


def _key_bytes():
    """Sample 0: the key tile 64 .. 127 has no visible byte; sample 1: one visible key."""
    g = torch.Generator().manual_seed(5)
    vis = torch.rand(2, MS, generator=g) > 0.3
    vis[0, 64:128] = False
    vis[0, 0] = True
    vis[1] = False
    vis[1, 3] = True
    return vis


def _image(per_head: bool):
    """A finite bias with -inf entries: one pattern for all heads, or a different one per head (column 0 and, for the
    sample with one visible key, column 3 stay finite: every row keeps a visible key)."""
    n = MH if per_head else 1
    a = rnd(n, MT, MS, seed=17) * 0.5
    i, j = torch.arange(MT)[:, None], torch.arange(MS)[None, :]
    for h in range(n):
        a[h][(i + 2 * j + h) % (h + 3) == 0] = NINF
    a[:, :, 0] = 0.25
    a[:, :, 3] = -0.5
    a[:, :, 70:75] = NINF
    return a if per_head else a[0]


FAMILIES = {"plain": dict(), "kmask": dict(kvis=True), "amask": dict(add=False), "hmask": dict(add=True),
            "kamask": dict(kvis=True, add=True)}


@DTYPES
@pytest.mark.parametrize("family", list(FAMILIES))
@pytest.mark.parametrize("dh", [25, 64])
def test_kernel_under_masks(dtype, family, dh):
    f = FAMILIES[family]
    kvis = _key_bytes() if f.get("kvis") else None
    add = _image(f["add"]) if "add" in f else None
    pr = Problem(dtype, 2, MH, MT, MS, dh, True, None, kvis=kvis, add=add, seed=3)
    pr.call(("attn_head_maps", "_hmask"), [pr.output(ldw=MS + 5)])
    pr.check(f"{family} dh {dh}")
    first = pr.flat.clone()
    if family == "hmask":                           # each head's zeros sit at its own pattern
        P = pr.maps().cpu()
        future = ((torch.arange(MS)[None, :] - torch.arange(MT)[:, None]) >= pr.off)
        for h in range(MH):
            assert torch.equal(P[0, h] == 0, torch.isinf(add[h]) | future), f"head {h}: zeros off its pattern"
        assert not torch.equal(P[0, 0] == 0, P[0, 1] == 0)
    if kvis is not None:
        P = pr.maps()
        assert (P[0, :, :, 64:128] == 0).all() and float((P[1, :, :, 3] - 1).abs().max()) <= tol(dtype)
    pr.call(("attn_head_maps", "_amask"), [pr.output(ldw=MS + 5)])           # again (the *_amask wrapper launches *_hmask)
    torch.cuda.synchronize()
    assert torch.equal(first, pr.flat), f"{family}: two calls differ"


# ---------------------------------------------------------------------------------------------------------------------
# 5. the reference's per-head probabilities (head_maps.npz)
# ---------------------------------------------------------------------------------------------------------------------
# (case, weights prefix, biprojection, d, heads, layers, T, S (0: forward(x)), attn_mask): tests/test_attn_maps_gpu.py's rows
CASES = [("x", "f5x.", False, 24, 4, 2, 7, 5, True), ("xn", "f5xn.", False, 24, 4, 2, 6, 6, False),
         ("x25", "f5x25.", False, 50, 2, 2, 8, 11, True), ("b", "f5b.", True, 24, 4, 2, 5, 8, True),
         ("sb", "f15sb.", True, 24, 4, 2, 7, 0, True),
         ("c130x70", "f16c130x70.", False, 50, 2, 2, 130, 70, True), ("c128", "f16c128.", False, 256, 2, 1, 70, 40, True),
         ("c256", "f16c256.", True, 512, 2, 1, 40, 70, True)]
F32_LIMIT = 2e-4
# Largest max-abs / relative-L2 error of a case's per-head maps against head_maps.npz, measured on the MI355X (rounded up to
# two digits; profiles/head_maps_errors.json); the limits are 2x these.
MEASURED = {
    "bf16.b": {"max_abs": 6.0e-03, "rel_l2": 4.1e-03},
    "bf16.c128": {"max_abs": 6.3e-04, "rel_l2": 2.1e-03},
    "bf16.c130x70": {"max_abs": 7.3e-04, "rel_l2": 2.1e-03},
    "bf16.c256": {"max_abs": 3.1e-02, "rel_l2": 1.2e-02},
    "bf16.mha.k1": {"max_abs": 1.5e-03, "rel_l2": 1.5e-03},
    "bf16.mha.k2": {"max_abs": 1.5e-03, "rel_l2": 7.8e-04},
    "bf16.mha.k3": {"max_abs": 1.9e-03, "rel_l2": 1.1e-03},
    "bf16.sb": {"max_abs": 1.7e-03, "rel_l2": 1.6e-03},
    "bf16.x": {"max_abs": 1.6e-03, "rel_l2": 1.7e-03},
    "bf16.x25": {"max_abs": 1.5e-03, "rel_l2": 1.9e-03},
    "bf16.xn": {"max_abs": 3.1e-03, "rel_l2": 1.8e-03},
    "bf16x3.b": {"max_abs": 5.4e-07, "rel_l2": 3.1e-07},
    "bf16x3.c128": {"max_abs": 1.2e-07, "rel_l2": 3.7e-07},
    "bf16x3.c130x70": {"max_abs": 8.2e-08, "rel_l2": 3.3e-07},
    "bf16x3.c256": {"max_abs": 7.9e-06, "rel_l2": 2.8e-06},
    "bf16x3.sb": {"max_abs": 1.2e-07, "rel_l2": 1.1e-07},
    "bf16x3.x": {"max_abs": 1.5e-07, "rel_l2": 1.7e-07},
    "bf16x3.x25": {"max_abs": 2.4e-07, "rel_l2": 2.2e-07},
    "bf16x3.xn": {"max_abs": 1.5e-07, "rel_l2": 1.9e-07},
}

_FIX = {}
_MEAS = {}
# where the measured errors go (the JSON of profiles/head_maps_errors.json): set BPMULT_ERROR_LOG to a file path to record
# them; unset, nothing is written
_LOG = os.environ.get("BPMULT_ERROR_LOG")


def load(name):
    if name not in _FIX:
        _FIX[name] = dict(np.load(os.path.join(G, name + ".npz")))
    return _FIX[name]


def _note(prec, tag, max_abs, rel):
    key = f"{prec}.{tag}"
    old = _MEAS.get(key, {"max_abs": 0.0, "rel_l2": 0.0})
    _MEAS[key] = {"max_abs": max(old["max_abs"], max_abs), "rel_l2": max(old["rel_l2"], rel)}
    if not _LOG:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(_LOG)), exist_ok=True)
        with open(_LOG, "w") as f:
            json.dump(_MEAS, f, indent=1, sort_keys=True)
    except OSError:
        pass


def _errors(got, ref):
    a, b = got.detach().double().cpu().numpy(), ref.astype(np.float64)
    assert a.shape == b.shape, (a.shape, b.shape)
    assert np.isfinite(a).all()
    return float(np.abs(a - b).max()), float(np.linalg.norm(a - b) / max(np.linalg.norm(b), 1e-12))


def _held(prec, tag, worst):
    _note(prec, tag, *worst)
    print(f"{prec} {tag}: max-abs {worst[0]:.3e} rel-L2 {worst[1]:.3e}")
    if prec == "f32":
        assert worst[0] <= F32_LIMIT, f"max err {worst[0]:.3e} > {F32_LIMIT:.1e}"
    else:
        lim = MEASURED[f"{prec}.{tag}"]
        assert worst[0] <= 2 * lim["max_abs"] and worst[1] <= 2 * lim["rel_l2"], \
            f"max-abs {worst[0]:.3e} (limit {2 * lim['max_abs']:.2e}), rel-L2 {worst[1]:.3e} (limit {2 * lim['rel_l2']:.2e})"


def _hidden(Tn, S, mask):
    if not mask:
        return np.zeros((Tn, S), dtype=bool)
    return (np.arange(S)[None, :] - np.arange(Tn)[:, None]) >= 1 + abs(S - Tn)


def _inputs(pfx, what, n, d):
    x = T(det(pfx + what, (n, B, d)))
    m = T(det(pfx + what + ".z", (n, B))) > 1.0
    x[:, :, 0][m] = 0.0
    return x


@pytest.mark.parametrize("prec", ["f32", "bf16x3", "bf16"])
@pytest.mark.parametrize("tag,pfx,bi,d,H,L,Tn,S,mask", CASES, ids=[c[0] for c in CASES])
def test_reference_standalone(prec, tag, pfx, bi, d, H, L, Tn, S, mask):
    g = load("head_maps")
    enc = TransformerEncoder(d, H, L, attn_mask=mask, biprojection=bi)
    enc.precision = prec
    with torch.no_grad():
        for k, p in enc.named_parameters():
            p.copy_(T(det_param(pfx + k, p.shape)))
    enc = enc.cuda().train()
    x = _inputs(pfx, "x", Tn, d)
    x[-2:] = 0.0
    with pytest.raises(RuntimeError, match="forward"):
        enc.attention_maps(per_head=True)
    if S:
        kv = _inputs(pfx, "kv", S, d).cuda()
        enc(x.cuda(), kv, kv)
    else:
        enc(x.cuda())
    before = enc.attention_maps()
    maps = enc.attention_maps(per_head=True)
    after = enc.attention_maps()
    blocks = (("self",) if bi or not S else ()) + (("cross",) if S else ())
    assert len(maps) == L
    worst = [0.0, 0.0]
    for i, m in enumerate(maps):
        assert tuple(m) == blocks
        for blk in blocks:
            ref = g[f"{tag}.L{i}.{blk}"]
            w = m[blk].weights
            assert m[blk].query_steps is None and w.dtype == torch.float32 and w.is_contiguous() and not w.requires_grad
            Sk = ref.shape[-1]
            assert tuple(w.shape) == (B, H, Tn, Sk)
            assert (w[:, :, T(_hidden(Tn, Sk, mask)).cuda()] == 0).all(), f"L{i}.{blk}: masked entries must be exactly 0"
            e, r = _errors(w, ref)
            worst = [max(worst[0], e), max(worst[1], r)]
            # per_head=False after per_head=True: the bits it returned before; and the head mean of the per-head maps
            assert torch.equal(before[i][blk].weights, after[i][blk].weights)
            assert float((w.mean(1) - after[i][blk].weights).abs().max()) <= SUM_LIMIT
    _held(prec, tag, worst)


def args_for(model, **kw):
    a = dict(model=model, orig_d_l=768, orig_d_v=35, orig_d_a=74, orig_d_p=4096, hidden_sz=300, vonly=True, lonly=True,
             aonly=True, num_heads=12, layers=8, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.,
             res_dropout=0., out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6,
             bert_model="unused", text_features=True)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.mark.skipif(os.environ.get("BPMULT_GRAPH", "1") == "0", reason="graph replay switched off by BPMULT_GRAPH=0")
@pytest.mark.parametrize("prune", [pytest.param(False, id="dense"), pytest.param(True, id="pruned")])
def test_reference_model(prune):
    """mmtrvat at F7's configuration, f32: after the first (eager) call and after the fourth (a graph replay)."""
    from bpmult_amd.models.bpmult import LEVEL2
    g = load("head_maps")
    rows, full = g["m.query_rows"], g["m.full"].tolist()
    model = get_model(args_for("mmtrvat", hidden_sz=24, num_heads=4, layers=2, orig_d_l=32))
    model.set_prune_unused_rows(prune)
    with torch.no_grad():
        for k, p in model.named_parameters():
            p.copy_(T(det_param("f7." + k, p.shape)))
    model.precision = "f32"
    model = model.cuda().train()
    xs = [T(det("f7.xl", (2, 50, 32))).cuda(), T(det("f7.img", (2, 500, 35))).cuda(), T(det("f7.aud", (2, 375, 74))).cuda()]
    with pytest.raises(RuntimeError, match="forward"):
        model.attention_maps(per_head=True)
    hidden = T(_hidden(512, 512, True)).cuda()
    for call in range(4):
        model(xs[0], None, None, xs[1], xs[2])
        if call not in (0, 3):
            continue
        if call == 3:
            assert any("graph" in e for e in model._trunks[2]._fg.values()), "the fourth call is a graph replay"
        maps = model.attention_maps(per_head=True)
        assert sorted(maps) == sorted(g["m.names"].tolist())
        for n, per_layer in maps.items():
            assert len(per_layer) == 2
            for i, m in enumerate(per_layer):
                assert tuple(m) == ("cross",)
                w, steps = m["cross"]
                if prune and n in LEVEL2:
                    assert steps == (0, 511) and tuple(w.shape) == (2, 4, 2, 512)
                    assert (w[:, :, 0, 1:] == 0).all()
                    if n in full:
                        e, _ = _errors(w, g[f"m.{n}.L{i}.rows"][:, :, [0, 7]])
                        assert e <= F32_LIMIT, f"call {call} {n}.L{i}: max err {e:.3e}"
                    continue
                assert steps is None and tuple(w.shape) == (2, 4, 512, 512)
                assert (w[:, :, hidden] == 0).all()
                if n in full:
                    e, _ = _errors(w[:, :, T(rows).cuda()], g[f"m.{n}.L{i}.rows"])
                    assert e <= F32_LIMIT, f"call {call} {n}.L{i}: max err {e:.3e}"
                # every head's (norm, sum): F15's check, per head
                wd = w.double()
                hn = torch.stack([wd.pow(2).sum(dim=(0, 2, 3)).sqrt(), wd.sum(dim=(0, 2, 3))], 1).cpu().numpy()
                ref = g[f"m.{n}.L{i}.hn"]
                err = np.maximum(np.abs(hn[:, 0] - ref[:, 0]), np.abs(hn[:, 1] - ref[:, 1]) / np.sqrt(2 * 512 * 512)) / ref[:, 0]
                assert (err <= F32_LIMIT).all(), f"call {call} {n}.L{i}: per-head norm / sum off by {err}"
        sel = model.attention_maps(names=["trans_a_with_v2l"], layers=[1], per_head=True)
        assert torch.equal(sel["trans_a_with_v2l"][0]["cross"].weights, maps["trans_a_with_v2l"][1]["cross"].weights)


def _mha(c, prec):
    tag, form, Tn, S, Bn, d, H = c[:7]
    x = mha_kpm_cases.inputs(c)
    m = MultiheadAttention(d, H, bias=c[9])
    m.precision = prec
    with torch.no_grad():
        for k, p in m.named_parameters():
            p.copy_(T(x[k]))
    m = m.cuda().eval()
    q = T(x["q"]).cuda()
    k = q if form == "qkv" else T(x["k"]).cuda()
    v = k if form != "sep" else T(x["v"]).cuda()
    mask = None if mha_kpm_cases.attn_mask(c) is None else T(mha_kpm_cases.attn_mask(c)).cuda()
    bias = None if mha_kpm_cases.learned_bias(c) is None else T(mha_kpm_cases.learned_bias(c)).cuda().requires_grad_(True)
    return m, q, k, v, mask, bias, T(mha_kpm_cases.padding(c)).cuda()


@pytest.mark.parametrize("prec", ["f32", "bf16"])
@pytest.mark.parametrize("tag", mha_kpm_cases.REFERENCE_RUNS)
def test_reference_multihead_attention(tag, prec):
    c = mha_kpm_cases.case(tag)
    ref = load("head_maps")[f"mha.{tag}"]
    m, q, k, v, mask, bias, kpm = _mha(c, prec)
    y, w = m(q, k, v, attn_mask=mask, attn_bias=bias, key_padding_mask=kpm, average_attn_weights=False)
    ya, wa = m(q, k, v, attn_mask=mask, attn_bias=bias, key_padding_mask=kpm)
    assert tuple(w.shape) == ref.shape and w.dtype == torch.float32 and w.is_contiguous() and not w.requires_grad and w.grad_fn is None
    assert torch.equal(y, ya) and float((w.mean(1) - wa).abs().max()) <= SUM_LIMIT
    assert (w[kpm[:, None, None, :].expand_as(w)] == 0).all() and (w[T(ref == 0).cuda()] == 0).all()
    _held(prec, "mha." + tag, list(_errors(w, ref)))
    y2, none = m(q, k, v, attn_mask=mask, attn_bias=bias, key_padding_mask=kpm, need_weights=False, average_attn_weights=False)
    assert none is None and torch.equal(y2, y)


@pytest.mark.parametrize("prec", ["f32", "bf16"])
def test_multihead_attention_families(prec, monkeypatch):
    """No mask, attn_mask, key_padding_mask, [H, T, S] bias beside a padding mask: each reaches its own per-head entry, the
    result is [B, H, T, S], its head mean is the averaged call's, rows sum to 1, backward() still runs."""
    c = mha_kpm_cases.case("k4")
    m, q, k, v, mask, bias, kpm = _mha(c, prec)
    seen = []
    for fn in ("attn_head_maps", "attn_head_maps_amask", "attn_head_maps_kmask", "attn_head_maps_kamask"):
        monkeypatch.setattr(ops, fn, (lambda real, name: lambda *a: (seen.append(name), real(*a))[1])(getattr(ops, fn), fn))
    for kw, entry in ((dict(), "attn_head_maps"), (dict(attn_mask=mask), "attn_head_maps_amask"), (dict(key_padding_mask=kpm), "attn_head_maps_kmask"),
                      (dict(attn_mask=mask, attn_bias=bias, key_padding_mask=kpm), "attn_head_maps_kamask")):
        del seen[:]
        qq = q.clone().requires_grad_(True)
        y, w = m(qq, k, v, average_attn_weights=False, **kw)
        assert seen == [entry]
        _, wa = m(qq, k, v, **kw)
        assert tuple(w.shape) == (c[4], c[6], c[2], c[3]) and not w.requires_grad
        assert float((w.mean(1) - wa).abs().max()) <= SUM_LIMIT
        assert float((w.double().sum(-1) - 1).abs().max()) <= tol(BPM_F32 if prec == "f32" else BPM_BF16)
        y, w = m(qq, k, v, average_attn_weights=False, **kw)
        y.sum().backward()
        assert torch.isfinite(qq.grad).all()


# ---------------------------------------------------------------------------------------------------------------------
# 6. properties
# ---------------------------------------------------------------------------------------------------------------------
DROP = dict(attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.25, out_dropout=0.1)      # README rates


def _toy(seed=3, **kw):
    torch.manual_seed(seed)
    m = get_model(args_for("mmtrvat", hidden_sz=24, num_heads=4, layers=2, orig_d_l=32, num_vectors_l=80, num_vectors_a=48,
                           num_vectors_v=72, **kw))
    with torch.no_grad():
        for p in m.parameters():
            if p.dim() == 1:
                p.add_(0.1 * torch.randn_like(p))
    return m


def _toy_inputs(seed=4):
    g = torch.Generator().manual_seed(seed)
    r = lambda *s: torch.randn(*s, generator=g).cuda()
    return [r(2, 17, 32), r(2, 48, 35), r(2, 31, 74)]


@pytest.mark.skipif(os.environ.get("BPMULT_GRAPH", "1") == "0", reason="graph replay switched off by BPMULT_GRAPH=0")
@pytest.mark.parametrize("graphs", [False, True], ids=["eager", "graph"])
def test_taking_per_head_maps_does_not_disturb_the_step(graphs):
    """forward + attention_maps(per_head=True) + backward against forward + backward on a copy of the model, README dropout
    rates on, four steps (with graphs: the later ones are replays): the comparison of
    tests/test_attn_maps_gpu.py::test_taking_the_maps_does_not_disturb_the_step.  Shapes and query_steps follow the pruned
    schedule (the default), and the averaged maps taken afterwards are the bits taken before."""
    from bpmult_amd.models.bpmult import LEVEL2
    m1 = _toy(**DROP)
    m1.precision = "bf16"
    m2 = copy.deepcopy(m1)
    m1, m2 = m1.cuda().train(), m2.cuda().train()
    m1.use_graphs = m2.use_graphs = graphs
    tgt = (torch.randn(2, 6, generator=torch.Generator().manual_seed(1)) > 0).float().cuda()
    x = _toy_inputs()
    for step in range(4):
        outs = []
        for m, take in ((m1, False), (m2, True)):
            for p in m.parameters():
                p.grad = None
            xs = [t.clone().requires_grad_(True) for t in x]
            logits, z = m(xs[0], None, None, *xs[1:], output_gate=True)
            if take:
                avg = m.attention_maps()
                maps = m.attention_maps(per_head=True)
                again = m.attention_maps()
                trunk = m._trunks[2]
                assert len(maps) == 12
                for n, per in maps.items():
                    for i, blocks in enumerate(per):
                        w, steps = blocks["cross"]
                        a = avg[n][i]["cross"]
                        assert steps == a.query_steps and tuple(w.shape) == (2, 4) + tuple(a.weights.shape[1:])
                        if n in LEVEL2:
                            Tfull = trunk.N[LEVEL2[n][0]]
                            assert steps == (0, Tfull - 1) and w.shape[2] == 2
                        assert torch.equal(a.weights, again[n][i]["cross"].weights)
                        assert float((w.mean(1) - a.weights).abs().max()) <= SUM_LIMIT
                        assert float((w.double().sum(-1) - 1).abs().max()) <= tol(BPM_BF16)
            loss = torch.nn.functional.binary_cross_entropy_with_logits(logits, tgt)
            loss.backward()
            outs.append((logits.detach().clone(), z.detach().clone(), loss.detach().clone(), [t.grad.clone() for t in xs],
                         {k: p.grad.detach().clone() for k, p in m.named_parameters() if p.grad is not None}))
        a, b = outs
        assert torch.equal(a[0], b[0]) and torch.equal(a[1], b[1]) and torch.equal(a[2], b[2]), f"step {step}"
        for u, v in zip(a[3], b[3]):
            assert torch.equal(u, v), f"step {step}: input gradients differ"
        assert a[4].keys() == b[4].keys()
        for k in a[4]:
            if "gmu." in k or k.startswith(("proj1", "proj2", "out_layer")) or "layer_norm" in k or "bias" in k:
                assert float((a[4][k] - b[4][k]).abs().max()) <= 1e-5 * max(1.0, float(a[4][k].abs().max())), (step, k)
            else:
                assert torch.equal(a[4][k], b[4][k]), f"step {step}: gradient of {k} differs"
    if graphs:
        assert any("graph" in e for e in m2._trunks[2]._fg.values())


def test_encoder_per_head_maps_under_padding_masks_and_after_backward():
    """A masked plan takes its per-head maps under the plan's key masks (exactly 0 at padded keys), and backward() leaves
    them bit-equal."""
    enc = TransformerEncoder(24, 4, 2, attn_dropout=0.1, res_dropout=0.1, attn_mask=True).cuda().train()
    x = rnd(9, 2, 24, seed=1).cuda().requires_grad_(True)
    kv = rnd(12, 2, 24, seed=2).cuda()
    kpm = torch.zeros(2, 12, dtype=torch.bool, device=DEV)
    kpm[1, 9:] = True
    y = enc(x, kv, kv, key_padding_mask=kpm)
    a = enc.attention_maps(per_head=True)
    avg = enc.attention_maps()
    assert a[0]["cross"].weights.shape == (2, 4, 9, 12)
    for i in range(2):
        w = a[i]["cross"].weights
        assert (w[1, :, :, 9:] == 0).all() and float((w.double().sum(-1) - 1).abs().max()) <= tol(BPM_BF16)
        assert float((w.mean(1) - avg[i]["cross"].weights).abs().max()) <= SUM_LIMIT
    y.sum().backward()
    c = enc.attention_maps(per_head=True)
    assert all(torch.equal(a[i]["cross"].weights, c[i]["cross"].weights) for i in range(2))
