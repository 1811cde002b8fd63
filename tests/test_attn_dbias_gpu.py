"""The gradient of the additive attention mask (bpm_attn_bwd_dbias) and the head stride of bpm_attn_hmask on the MI355X, through
`ops`, with the harness of tests/test_attn_amask_gpu.py: its inputs (same seeds, CT-rounded), its masks, its NaN-padded mask
allocations and its fp64 restatement -- here with the mask as an autograd leaf, so mask.grad is the reference d(bias).

Forms: `shared` (one [T, S] image, stride 0, gradient summed over samples and heads) and `head` (H different images through
the head stride -- forward, dQ, dK / dV and the maps read them -- gradient summed over samples, [H, T, S]).

Limits.  dB in f32: 1e-4 * max(1, |ref|max), that file's backward limit (dS is an intermediate of the dQ it holds to that).
dB in bf16: relative L2 <= BF16_DB_LIMIT = 2 x the maximum measured on the MI355X over the cases below
(profiles/attn_dbias_errors.json, written through BPMULT_ERROR_LOG), and the max error never above that file's 4e-2 * scale.
O / lse / dQ / dK / dV / maps of the per-head form: that file's limits.  Exact conditions (== 0 at hidden pairs, untouched
pad columns, run-to-run bit-equality) are asserted with ==."""
import json
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

import test_attn_amask_gpu as A  # noqa: E402  (the harness; none of its tests is imported by name)
from bpmult_amd import ops  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402

DEV = "cuda"
SHAPES = [(5, 5, 32), (64, 64, 64), (65, 67, 96), (130, 67, 64), (65, 65, 160)]
KINDS = ["finite", "mixed", "causal+finite"]
FORMS = ["shared", "head"]
NINF = float("-inf")
SENTINEL = 777.0
BF16_DB_LIMIT = 1.57e-2       # 2 x 7.85e-3, the maximum over the cases (5 x 5 x 32, causal+finite, per head: profiles/attn_dbias_errors.json)

_MEASURED = {}
_LOG = os.environ.get("BPMULT_ERROR_LOG")


def _note(key, rel, err):
    m = _MEASURED.setdefault(key, {"rel_l2": 0.0, "max_abs": 0.0})
    m["rel_l2"], m["max_abs"] = max(m["rel_l2"], rel), max(m["max_abs"], err)
    if not _LOG:
        return
    try:
        os.makedirs(os.path.dirname(os.path.abspath(_LOG)), exist_ok=True)
        json.dump(_MEASURED, open(_LOG, "w"), indent=1, sort_keys=True)
    except OSError:
        pass


def setup(dtype, T, S, dh, B=3, H=2):
    """A.setup for any (B, H): the same generators and rounding (identical tensors at B, H = 3, 2)."""
    dhp, ctt = A.dhp_for(dh), ops.ct_torch(dtype)

    def heads(x):
        buf = torch.zeros(*x.shape[:3], dhp, dtype=ctt)
        buf[..., :dh] = x.to(ctt)
        return buf.to(DEV), buf[..., :dh].double()

    Q, q = heads(A.rnd(B, H, T, dh, seed=21) * dh ** -0.5)
    K, k = heads(A.rnd(B, H, S, dh, seed=22))
    V, v = heads(A.rnd(B, H, S, dh, seed=23))
    dO, do = heads(A.rnd(B, H, T, dh, seed=24))
    return dict(dhp=dhp, ctt=ctt, d=H * dh, ld=pad32(H * dh), B=B, H=H, Q=Q, K=K, V=V, dO=dO, q=q, k=k, v=v, do=do)


def make_masks(kind, T, S, form, H=2):
    """fp32 [1, T, S] (shared) or [H, T, S] on the CPU: head h gets A.make_mask's image with its columns rotated by 5 h
    and its finite values scaled by 1 + h / 4 -- another image, and every row keeps its visible key."""
    base = A.make_mask(kind, T, S)
    if form == "shared":
        return base[None]
    return torch.stack([torch.roll(base, 5 * h, dims=1) * (1.0 + 0.25 * h) for h in range(H)])


def padded_images(m, extra, gap):
    """[N, R, C] -> device allocation of N images [R, ld], ld = C rounded up to 4 plus `extra`, `gap` floats between the
    images, NaN in every pad column and gap; -> (tensor, ld, head stride)."""
    N, R, Cn = m.shape
    ld = (Cn + 3) // 4 * 4 + extra
    hs = R * ld + gap
    buf = torch.full((N, hs), float("nan"))
    buf[:, :R * ld].view(N, R, ld)[:, :, :Cn] = m
    return buf.to(DEV), ld, hs


def device_masks(m):
    md, ldm, hs = padded_images(m, 4, 8)
    mt, ldt, hst = padded_images(m.transpose(1, 2).contiguous(), 8, 4)
    if m.shape[0] == 1:
        hs = hst = 0
    return ops.attn_amasks([(md, ldm, mt, ldt, hs, hst)]), (md, mt)


def alloc_db(nimg, T, S):
    lddb = (S + 3) // 4 * 4 + 4
    hs = T * lddb + 8
    buf = torch.full((nimg, hs), SENTINEL, device=DEV)
    return buf, lddb, (hs if nimg > 1 else 0)


def read_db(buf, lddb, T, S):
    """-> the gradient [nimg, T, S] on the CPU, after checking that nothing else was written."""
    b = buf.cpu()
    img = b[:, :T * lddb].view(-1, T, lddb)
    assert (img[:, :, S:] == SENTINEL).all(), "columns >= S of dB were written"
    assert (b[:, T * lddb:] == SENTINEL).all(), "the gap between the head images of dB was written"
    return img[:, :, :S]


def problem(dtype, s, T, S, dh, off, pdrop):
    B, H, ld, ctt = s["B"], s["H"], s["ld"], s["ctt"]
    O = torch.zeros(T * B, ld, device=DEV, dtype=ctt)
    lse, delta = torch.zeros(B, H, T, device=DEV), torch.zeros(B, H, T, device=DEV)
    dQ, dK, dV = (torch.full((L * B, ld), 7.0, device=DEV, dtype=ctt) for L in (T, S, S))
    p = ops.attn_problem(s["Q"], s["K"], s["V"], O, ld, lse, B, H, T, S, dh, s["dhp"], off, dO=s["dO"], delta=delta, dQ=dQ, lddq=ld,
                         dK=dK, lddk=ld, dV=dV, lddv=ld, dq_scale=1.0, drop_p=pdrop, drop_site=3)
    return p, (O, lse, dQ, dK, dV, delta)


def run(dtype, s, T, S, dh, off, am, form, pdrop=0.0, seed=9, maps=False):
    """Forward, dQ, dK / dV [, maps] under the masks `am`, then the bias gradient in `form`.
    -> (O, lse, dQ, dK, dV), W or None, dB [nimg, T, S] (CPU), workspace bytes."""
    B, H = s["B"], s["H"]
    p, outs = problem(dtype, s, T, S, dh, off, pdrop)
    ops.attn_fwd_amask(dtype, [p], am[0], seed=seed)
    ops.attn_bwd_dq_amask(dtype, [p], am[0], seed=seed)
    ops.attn_bwd_dkv_amask(dtype, [p], am[0], seed=seed)
    W = None
    if maps:
        W = torch.full((B, T, S + 3), 5.0, device=DEV)
        ops.attn_maps_amask(dtype, [ops.attn_map_problem(s["Q"], s["K"], outs[1], W, S + 3, B, H, T, S, dh, s["dhp"], off)], am[0])
    buf, lddb, hs = alloc_db(H if form == "head" else 1, T, S)
    db = ops.attn_dbias([(buf, lddb, hs)])
    nws = ops.attn_dbias_ws_bytes([p], db)
    ws = torch.full(((nws + 3) // 4,), float("nan"), device=DEV) if nws else None
    ops.attn_bwd_dbias(dtype, [p], am[0], db, seed=seed, ws=ws)
    torch.cuda.synchronize()
    return outs[:5], W, read_db(buf, lddb, T, S), nws


_REF = {}


def reference(dtype, T, S, dh, kind, form, B=3, H=2):
    """fp64 restatement on the CT-rounded inputs with the mask as a leaf, computed once per case."""
    key = (dtype, T, S, dh, kind, form, B, H)
    if key not in _REF:
        s = setup(dtype, T, S, dh, B, H)
        masks = make_masks(kind, T, S, form, H)
        off = 1 + abs(S - T) if kind == "causal+finite" else 0
        q, k, v = (s[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        ml = masks.double().requires_grad_(True)
        sc = q @ k.transpose(-1, -2) + ml[None]
        if off > 0:
            sc = sc.masked_fill(((torch.arange(S)[None, :] - torch.arange(T)[:, None]) >= off)[None, None], NINF)
        pr = torch.softmax(sc, -1)
        o_ref, lse_ref = pr @ v, torch.logsumexp(sc, -1)
        (o_ref * s["do"]).sum().backward()
        hidden = torch.isinf(sc.detach())[0]                             # [H, T, S], the same in every sample
        if form == "shared":
            assert bool((hidden == hidden[:1]).all())
            hidden = hidden[:1]
        _REF[key] = (s, masks, off, o_ref.detach(), lse_ref.detach(), q.grad, k.grad, v.grad, pr.detach().mean(1), hidden, ml.grad)
    return _REF[key]


def check_db(dtype, db, db_ref, hidden, what):
    assert db.shape == db_ref.shape, (db.shape, db_ref.shape)
    assert torch.isfinite(db).all(), what + ": non-finite"
    assert (db[hidden] == 0).all(), what + ": the gradient of a hidden pair must be exactly 0.0f"
    assert float(db_ref.abs().max()) > 0
    scale = max(1.0, db_ref.abs().max().item())
    err = (db.double() - db_ref).abs().max().item()
    rel = ((db.double() - db_ref).norm() / db_ref.norm()).item()
    print(f"{what}: max err {err:.3e} (scale {scale:.3g}), rel-L2 {rel:.3e}")
    if dtype == BPM_F32:
        assert err <= 1e-4 * scale, f"{what}: max err {err:.3e} > {1e-4 * scale:.3e}"
    else:
        _note(what, rel, err)
        assert rel <= BF16_DB_LIMIT and err <= 4e-2 * scale, f"{what}: rel-L2 {rel:.3e} (limit {BF16_DB_LIMIT:.1e}), max err {err:.3e} (limit {4e-2 * scale:.3e})"


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
@pytest.mark.parametrize("form", FORMS)
def test_bias_gradient_matches_fp64(dtype, T, S, dh, kind, form):
    s, masks, off, o_ref, lse_ref, dq_ref, dk_ref, dv_ref, w_ref, hidden, db_ref = reference(dtype, T, S, dh, kind, form)
    B, H, d = s["B"], s["H"], s["d"]
    am = device_masks(masks)
    (O, lse, dQ, dK, dV), W, db, nws = run(dtype, s, T, S, dh, off, am, form, maps=form == "head")
    # B * H = 6 heads: the shared form splits them over two workgroups per tile, the per-head form (3 samples) does not
    assert (nws > 0) == (form == "shared"), "these cases are meant to take both the split and the unsplit launch"
    check_db(dtype, db, db_ref, hidden, f"{'f32' if dtype == BPM_F32 else 'bf16'}.{T}x{S}x{dh}.{kind}.{form}")
    if form != "head":
        return

    def rows(x, L):
        return x[:, :d].float().reshape(L, B, H, dh).permute(1, 2, 0, 3)

    t, tb, tm = (3e-5, 1e-4, 2e-5) if dtype == BPM_F32 else (2e-2, 4e-2, 1.5e-2)
    A.close(rows(O, T), o_ref, t, "O")
    A.close(lse, lse_ref, t, "lse")
    A.close(rows(dQ, T), dq_ref, tb, "dQ")
    A.close(rows(dK, S), dk_ref, tb, "dK")
    A.close(rows(dV, S), dv_ref, tb, "dV")
    Wc = W.cpu()
    assert (Wc[:, :, S:] == 5.0).all(), "the maps kernel wrote past column S"
    w = Wc[:, :, :S]
    err = (w.double() - w_ref).abs().max().item()
    assert torch.isfinite(w).all() and err <= tm, f"maps: max err {err:.3e} > {tm:.1e}"
    assert (w[hidden.all(0)[None].expand(B, T, S)] == 0).all(), "a map entry hidden in every head must be exactly 0.0f"
    assert (w.double().sum(-1) - 1.0).abs().max().item() <= tm


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
def test_thirty_six_heads_split_over_nine_workgroups_per_tile(dtype):
    T = S = 65
    dh, B, H = 64, 9, 4
    s, masks, off, *_, hidden, db_ref = reference(dtype, T, S, dh, "mixed", "shared", B, H)
    am = device_masks(masks)
    _, _, db, nws = run(dtype, s, T, S, dh, off, am, "shared")
    assert nws == 9 * T * 68 * 4, "36 heads, 4 tiles: nine splits of four heads, one [T, ldp] partial image each"
    check_db(dtype, db, db_ref, hidden, f"{'f32' if dtype == BPM_F32 else 'bf16'}.36heads.shared")


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("form", FORMS)
@pytest.mark.parametrize("pdrop", [0.0, 0.1])
def test_same_seed_twice_is_bit_equal(dtype, form, pdrop):
    T, S, dh = 130, 67, 64
    s = setup(dtype, T, S, dh)
    am = device_masks(make_masks("mixed", T, S, form))
    a = run(dtype, s, T, S, dh, 0, am, form, pdrop)
    b = run(dtype, s, T, S, dh, 0, am, form, pdrop)
    assert torch.equal(a[2], b[2]) and torch.isfinite(a[2]).all()
    for x, y in zip(a[0], b[0]):
        assert torch.equal(x, y)
    if pdrop > 0:
        c = run(dtype, s, T, S, dh, 0, am, form, pdrop, seed=10)
        assert not torch.equal(c[2], a[2]), "another seed must draw another dropout mask"


@pytest.mark.parametrize("T,S,dh", [(65, 68, 64), (64, 64, 64)])
def test_with_dropout_it_sums_the_score_gradient_the_dq_pass_used(T, S, dh):
    """f32, all-zeros mask, drop_p = 0.1: no fp64 reference knows the keep mask, but the unmasked dQ entry exports the dS it
    multiplied by K.  dB must be its sum over the samples (per head) and over samples and heads (shared)."""
    dtype, pdrop, seed = BPM_F32, 0.1, 9
    s = setup(dtype, T, S, dh)
    B, H = s["B"], s["H"]
    p, (O, lse, dQ, dK, dV, delta) = problem(dtype, s, T, S, dh, 0, pdrop)
    dS, Pd = torch.zeros(B, H, T, S, device=DEV), torch.zeros(B, H, T, S, device=DEV)
    px = ops.attn_problem(s["Q"], s["K"], s["V"], O, s["ld"], lse, B, H, T, S, dh, s["dhp"], 0, dO=s["dO"], delta=delta, dQ=dQ,
                          lddq=s["ld"], dq_scale=1.0, drop_p=pdrop, drop_site=3, dS=dS, Pd=Pd, xs=(H * T * S, T * S, S))
    ops.attn_fwd(dtype, [p], seed=seed)
    ops.attn_bwd_dq(dtype, [px], seed=seed)
    am = device_masks(torch.zeros(1, T, S))
    assert float((Pd == 0).float().mean()) > 0.05, "dropout must have dropped something"
    for form in FORMS:
        buf, lddb, hs = alloc_db(H if form == "head" else 1, T, S)
        db = ops.attn_dbias([(buf, lddb, hs)])
        nws = ops.attn_dbias_ws_bytes([p], db)
        ws = torch.empty((nws + 3) // 4, device=DEV) if nws else None
        ops.attn_bwd_dbias(dtype, [p], am[0], db, seed=seed, ws=ws)
        torch.cuda.synchronize()
        got = read_db(buf, lddb, T, S).double()
        ref = dS.double().cpu().sum(0) if form == "head" else dS.double().cpu().sum((0, 1))[None]
        scale = max(1.0, ref.abs().max().item())
        err = (got - ref).abs().max().item()
        print(f"{form}: max err {err:.3e} (limit {1e-4 * scale:.3e})")
        assert float(ref.abs().max()) > 0 and err <= 1e-4 * scale, f"{form}: {err:.3e} > {1e-4 * scale:.3e}"


def test_head_stride_with_one_repeated_image_is_bit_equal_to_stride_zero():
    """H copies of one image through the head stride: forward, dQ, dK / dV and the maps equal the stride-0 results bit for
    bit, and the per-head gradients are the terms of the shared one."""
    dtype, (T, S, dh) = BPM_BF16, (65, 67, 96)
    s = setup(dtype, T, S, dh)
    m = make_masks("mixed", T, S, "shared")
    a = run(dtype, s, T, S, dh, 0, device_masks(m), "shared", 0.1, maps=True)
    b = run(dtype, s, T, S, dh, 0, device_masks(m.expand(s["H"], T, S).contiguous()), "head", 0.1, maps=True)
    for x, y, nm in zip(a[0] + (a[1],), b[0] + (b[1],), ("O", "lse", "dQ", "dK", "dV", "W")):
        assert torch.equal(x, y), nm
    ref = b[2].double().sum(0, keepdim=True)
    assert float((a[2].double() - ref).abs().max()) <= 1e-5 * max(1.0, float(ref.abs().max()))
