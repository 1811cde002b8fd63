"""Attention with a per-key byte mask AND an additive mask together (bpm_attn_fwd_kamask / _bwd_dq_kamask / _bwd_dkv_kamask /
bpm_attn_maps_kamask), the byte mask in the maps and bias-gradient kernels (bpm_attn_maps_kmask, bpm_attn_bwd_dbias_kmask), on
the MI355X through `ops`.

Bit-equality needs no tolerance: an all-ones byte mask gives the *_hmask entries' bits (shared and per-head image), an
all-zeros image the *_kmask entries', in f32 and bf16, with and without dropout.
Against an fp64 torch restatement (scores + image, -inf at the keys the sample's bytes hide, softmax, P V, autograd) the
limits are those of tests/test_attn_amask_gpu.py (its header, lines 3-4), relative to max(1, |ref|max): forward and lse
3e-5 (f32) / 2e-2 (bf16), dQ / dK / dV and the bias gradient 1e-4 / 4e-2, the maps 2e-5 / 1.5e-2 absolute.  The exact
conditions (zero dK / dV rows and map entries of a hidden key, a zero bias gradient at a key hidden in every sample) are
asserted with ==.

The additive image is allocated wider than S (its transpose wider than T) with NaN in the pad columns, and the byte mask
wider than S with visible (1) bytes there: whatever sits in the pads must never reach a result."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import ops  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402

DEV = "cuda"
B, H = 3, 2
NINF = float("-inf")
EQ_SHAPES = [(65, 65, 64), (130, 132, 32), (65, 68, 160), (65, 68, 200)]
REF_SHAPES = [(T, S, dh) for (T, S) in ((5, 5), (64, 64), (65, 65), (130, 67)) for dh in (32, 64)] + [(65, 67, 96), (65, 67, 200)]
PATTERNS = ["suffix", "first_tile", "scattered"]
KINDS = ["finite", "holes"]
NAMES = ("O", "lse", "dQ", "delta", "dK", "dV")


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def close(got, ref, t, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite"
    scale = max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    print(f"{what}: max err {err:.3e} (limit {t * scale:.3e})")
    assert err <= t * scale, f"{what}: max err {err:.3e} vs tol {t * scale:.3e}"


def make_bytes(pattern, S):
    """bool [B, S] on the CPU, True = visible.  suffix: ragged padded suffixes, sample 0 unpadded; first_tile: the first 64
    keys of the last sample hidden (S > 64; a short prefix otherwise); scattered: a random half, another per sample.  Key
    S - 1 is hidden in every sample of `scattered`."""
    vis = torch.ones(B, S, dtype=torch.bool)
    if pattern == "suffix":
        vis[1, max(1, S - 3):] = False
        vis[2, max(1, S // 2):] = False
    elif pattern == "first_tile":
        vis[1, max(1, S - 2):] = False
        vis[2, :min(64, S - 1)] = False
    else:
        vis = torch.rand(B, S, generator=torch.Generator().manual_seed(77 + S)) < 0.5
        vis[:, 0] = True
        if S > 1:
            vis[:, S - 1] = False
    assert vis.any(1).all()
    return vis


def make_image(kind, T, S, vis, heads=1):
    """fp32 [heads, T, S] on the CPU; holes: 40 % -inf, repaired so that every (sample, head, row) keeps a visible key."""
    g = torch.Generator().manual_seed(1000 * T + S + heads)
    m = 2.0 * torch.randn(heads, T, S, generator=g)
    if kind == "holes":
        m[torch.rand(heads, T, S, generator=g) < 0.4] = NINF
        for b in range(B):                          # the first visible key of every sample stays finite in every row
            col = m[:, :, int(vis[b].nonzero()[0])]
            col[torch.isinf(col)] = 0.0
    assert (torch.isfinite(m)[None] & vis[:, None, None, :]).any(-1).all()
    return m


def device_image(m):
    """[heads, T, S] -> ops.attn_amasks descriptors of NaN-padded device allocations (and the tensors, to keep them alive)."""
    heads, T, S = m.shape
    ldm, ldt = (S + 3) // 4 * 4 + 4, (T + 3) // 4 * 4 + 8
    md, mt = torch.full((heads, T, ldm), float("nan")), torch.full((heads, S, ldt), float("nan"))
    md[:, :, :S], mt[:, :, :T] = m, m.transpose(1, 2)
    md, mt = md.to(DEV), mt.to(DEV)
    desc = (md, ldm, mt, ldt) if heads == 1 else (md, ldm, mt, ldt, T * ldm, S * ldt)
    return ops.attn_amasks([desc]), (md, mt)


def device_bytes(vis):
    """bool [B, S] -> ops.attn_kmasks descriptors of a [B, S + 5] allocation whose pad bytes say `visible`."""
    S = vis.shape[1]
    buf = torch.ones(B, S + 5, dtype=torch.uint8)
    buf[:, :S] = vis.to(torch.uint8) * 3            # any nonzero byte means visible
    buf = buf.to(DEV)
    return ops.attn_kmasks([(buf, S + 5)]), buf


def dhp_for(dh):
    return 32 if dh <= 32 else 64 if dh <= 64 else 128 if dh <= 128 else 256


_SETUP = {}


def setup(dtype, T, S, dh):
    key = (dtype, T, S, dh)
    if key not in _SETUP:
        dhp, ctt, d = dhp_for(dh), ops.ct_torch(dtype), H * dh

        def heads(x):        # [B,H,L,dh] cpu -> device CT [B,H,L,dhp], and the CT-rounded values
            buf = torch.zeros(*x.shape[:3], dhp, dtype=ctt)
            buf[..., :dh] = x.to(ctt)
            return buf.to(DEV), buf[..., :dh].double()

        Q, q = heads(rnd(B, H, T, dh, seed=21) * dh ** -0.5)
        K, k = heads(rnd(B, H, S, dh, seed=22))
        V, v = heads(rnd(B, H, S, dh, seed=23))
        dO, do = heads(rnd(B, H, T, dh, seed=24))
        _SETUP[key] = dict(dhp=dhp, ctt=ctt, d=d, ld=pad32(d), Q=Q, K=K, V=V, dO=dO, q=q, k=k, v=v, do=do)
    return _SETUP[key]


def run(dtype, s, T, S, dh, km=None, am=None, pdrop=0.0, seed=9, maps=True, dbias=None, dbias_km="same"):
    """Forward, dQ, dK / dV through the family (km, am) select [, maps] [, the bias gradient with `dbias` images; dbias_km:
    the byte masks that launch takes, default km].  -> {O, lse, dQ, delta, dK, dV [, W] [, dB]} (device tensors)."""
    ld, ctt = s["ld"], s["ctt"]
    O = torch.zeros(T * B, ld, device=DEV, dtype=ctt)
    lse, delta = torch.zeros(B, H, T, device=DEV), torch.zeros(B, H, T, device=DEV)
    dQ, dK, dV = (torch.full((L * B, ld), 7.0, device=DEV, dtype=ctt) for L in (T, S, S))
    p = ops.attn_problem(s["Q"], s["K"], s["V"], O, ld, lse, B, H, T, S, dh, s["dhp"], 0, dO=s["dO"], delta=delta, dQ=dQ, lddq=ld,
                         dK=dK, lddk=ld, dV=dV, lddv=ld, dq_scale=1.0, drop_p=pdrop, drop_site=3)
    W = torch.full((B, T, S + 3), 5.0, device=DEV)
    mp = ops.attn_map_problem(s["Q"], s["K"], lse, W, S + 3, B, H, T, S, dh, s["dhp"], 0)
    if km is None and am is None:
        family, beside = "", ()
    elif km is None:
        family, beside = "_amask", (am[0],)           # launches the *_hmask entries
    elif am is None:
        family, beside = "_kmask", (km[0],)
    else:
        family, beside = "_kamask", (km[0], am[0])
    for which in ("fwd", "bwd_dq", "bwd_dkv"):
        getattr(ops, f"attn_{which}{family}")(dtype, [p], *beside, seed=seed)
    if maps:
        getattr(ops, f"attn_maps{family}")(dtype, [mp], *beside)
    out = dict(O=O, lse=lse, dQ=dQ, delta=delta, dK=dK, dV=dV)
    if maps:
        out["W"] = W
    if dbias is not None:
        lddb = (S + 3) // 4 * 4 + 4
        buf = torch.full((dbias, T, lddb), 777.0, device=DEV)
        db = ops.attn_dbias([(buf, lddb, T * lddb if dbias > 1 else 0)])
        nws = ops.attn_dbias_ws_bytes([p], db)
        ws = torch.full(((nws + 3) // 4,), float("nan"), device=DEV) if nws else None
        dkm = km if dbias_km == "same" else dbias_km
        ops.attn_bwd_dbias(dtype, [p], am[0], db, seed=seed, ws=ws, kmasks=None if dkm is None else dkm[0])
        out["dB"] = buf
    torch.cuda.synchronize()
    return out


def same_bits(a, b, names, what):
    for n in names:
        assert torch.equal(a[n], b[n]), f"{what}: {n} differs"


# --- bit-equality ------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh", EQ_SHAPES)
@pytest.mark.parametrize("pdrop", [0.0, 0.1])
@pytest.mark.parametrize("heads", [1, H])
def test_all_ones_bytes_are_bit_equal_to_the_hmask_entries(dtype, T, S, dh, pdrop, heads):
    """O, lse, dQ, delta, dK, dV, the maps and the bias gradient (bpm_attn_bwd_dbias_kmask with all ones, and with NULL,
    against bpm_attn_bwd_dbias), under a shared and a per-head image with holes."""
    s = setup(dtype, T, S, dh)
    ones = torch.ones(B, S, dtype=torch.bool)
    am = device_image(make_image("holes", T, S, ones, heads))
    km = device_bytes(ones)
    a = run(dtype, s, T, S, dh, None, am, pdrop, dbias=heads)
    b = run(dtype, s, T, S, dh, km, am, pdrop, dbias=heads)
    same_bits(a, b, NAMES + ("W", "dB"), "all-ones bytes vs *_hmask")
    c = run(dtype, s, T, S, dh, km, am, pdrop, maps=False, dbias=heads, dbias_km=None)       # kmasks = NULL after the kamask passes
    same_bits(a, c, ("dB",), "NULL byte masks vs bpm_attn_bwd_dbias")
    assert torch.isfinite(a["dB"][:, :, :S]).all() and (a["dB"][:, :, S:] == 777.0).all()


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh", EQ_SHAPES)
@pytest.mark.parametrize("pdrop", [0.0, 0.1])
def test_an_all_zeros_image_is_bit_equal_to_the_kmask_entries(dtype, T, S, dh, pdrop):
    """... and bpm_attn_maps_kamask with zeros equals bpm_attn_maps_kmask."""
    s = setup(dtype, T, S, dh)
    km = device_bytes(make_bytes("first_tile", S))
    am = device_image(torch.zeros(1, T, S))
    a = run(dtype, s, T, S, dh, km, None, pdrop)
    b = run(dtype, s, T, S, dh, km, am, pdrop)
    same_bits(a, b, NAMES + ("W",), "all-zeros image vs *_kmask")


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh", EQ_SHAPES)
def test_maps_kmask_with_all_ones_equals_maps(dtype, T, S, dh):
    s = setup(dtype, T, S, dh)
    a = run(dtype, s, T, S, dh)
    b = run(dtype, s, T, S, dh, device_bytes(torch.ones(B, S, dtype=torch.bool)))
    same_bits(a, b, NAMES + ("W",), "all-ones bytes vs the unmasked entries")


# --- against fp64 ------------------------------------------------------------------------------------------------------------
_REF = {}


def reference(dtype, T, S, dh, pattern, kind):
    """fp64 restatement on the CT-rounded inputs, computed once per case: a shared [T, S] image as an autograd leaf."""
    key = (dtype, T, S, dh, pattern, kind)
    if key not in _REF:
        s = setup(dtype, T, S, dh)
        vis = make_bytes(pattern, S)
        img = make_image(kind, T, S, vis)
        q, k, v = (s[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        bias = img[0].double().requires_grad_(True)
        sc = (q @ k.transpose(-1, -2) + bias).masked_fill(~vis[:, None, None, :], NINF)
        pr = torch.softmax(sc, -1)
        o_ref, lse_ref = pr @ v, torch.logsumexp(sc, -1)
        (o_ref * s["do"]).sum().backward()
        _REF[key] = (s, vis, img, o_ref.detach(), lse_ref.detach(), q.grad, k.grad, v.grad, pr.detach().mean(1), bias.grad,
                     torch.isinf(sc.detach()).all(1))                        # [B, T, S]: hidden in every head
    return _REF[key]


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh", REF_SHAPES)
@pytest.mark.parametrize("pattern", PATTERNS)
@pytest.mark.parametrize("kind", KINDS)
def test_both_masks_match_fp64(dtype, T, S, dh, pattern, kind):
    s, vis, img, o_ref, lse_ref, dq_ref, dk_ref, dv_ref, w_ref, db_ref, hidden = reference(dtype, T, S, dh, pattern, kind)
    r = run(dtype, s, T, S, dh, device_bytes(vis), device_image(img), dbias=1)
    d = s["d"]

    def rows(x, L):      # row-major [(l*B+b), h*dh+c] -> [B,H,L,dh]
        return x[:, :d].float().reshape(L, B, H, dh).permute(1, 2, 0, 3)

    t = 3e-5 if dtype == BPM_F32 else 2e-2
    tb = 1e-4 if dtype == BPM_F32 else 4e-2
    close(rows(r["O"], T), o_ref, t, "O")
    close(r["lse"], lse_ref, t, "lse")
    close(rows(r["dQ"], T), dq_ref, tb, "dQ")
    close(rows(r["dK"], S), dk_ref, tb, "dK")
    close(rows(r["dV"], S), dv_ref, tb, "dV")
    dB = r["dB"].cpu()
    assert (dB[:, :, S:] == 777.0).all(), "the bias-gradient kernel wrote past column S"
    close(dB[0, :, :S], db_ref, tb, "dB")
    # exact: a key its sample's byte hides gets zero dK / dV rows in that sample, and a zero map column
    dk4, dv4 = rows(r["dK"], S).cpu(), rows(r["dV"], S).cpu()                # [B,H,S,dh]
    gone = (~vis)[:, None, :, None].expand_as(dk4)
    assert (dk4[gone] == 0).all() and (dv4[gone] == 0).all(), "dK / dV rows of a hidden key must be exact zeros"
    tm = 2e-5 if dtype == BPM_F32 else 1.5e-2
    Wc = r["W"].cpu()
    assert (Wc[:, :, S:] == 5.0).all(), "the maps kernel wrote past column S"
    w = Wc[:, :, :S]
    assert torch.isfinite(w).all()
    err = (w.double() - w_ref).abs().max().item()
    print(f"maps: max err {err:.3e} (limit {tm:.1e})")
    assert err <= tm, f"maps: max err {err:.3e} > {tm:.1e}"
    assert (w[hidden] == 0).all(), "a hidden map entry must be exactly 0.0f"
    assert (w[(~vis)[:, None, :].expand(B, T, S)] == 0).all(), "a key the byte mask hides must be exactly 0.0f in the map"
    rs = (w.double().sum(-1) - 1.0).abs().max().item()
    assert rs <= tm, f"maps: row sums off by {rs:.3e}"
    # exact: no sample contributes at a key hidden in all of them
    never = (~vis).all(0)
    if never.any():
        assert (dB[0, :, :S][:, never] == 0).all(), "the bias gradient at a key hidden in every sample must be exactly 0"
    assert (dB[0, :, :S][hidden.all(0)] == 0).all()


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
def test_same_seed_twice_is_bit_equal_another_seed_differs(dtype):
    T, S, dh = 130, 67, 64
    s = setup(dtype, T, S, dh)
    vis = make_bytes("scattered", S)
    km, am = device_bytes(vis), device_image(make_image("holes", T, S, vis, H))
    a = run(dtype, s, T, S, dh, km, am, 0.1, dbias=H)
    b = run(dtype, s, T, S, dh, km, am, 0.1, dbias=H)
    same_bits(a, b, NAMES + ("W", "dB"), "same seed")
    for n in NAMES + ("W",):
        assert torch.isfinite(a[n].float()).all(), n
    c = run(dtype, s, T, S, dh, km, am, 0.1, seed=10, dbias=H)
    assert not torch.equal(c["O"], a["O"]) and not torch.equal(c["dB"], a["dB"]), "another seed must draw another dropout mask"
