"""Attention with an arbitrary additive mask (bpm_attn_fwd_amask / _bwd_dq_amask / _bwd_dkv_amask / bpm_attn_maps_amask) on
the MI355X against an fp64 torch restatement: scores + mask, softmax, P V, autograd for dQ / dK / dV.  Tolerances are the
ones tests/test_attn_kmask_gpu.py applies (forward and lse 3e-5 / 2e-2, backward 1e-4 / 4e-2 for f32 / bf16, relative to
max(1, |ref|max)); the maps are held to tests/test_attn_maps_gpu.py's `tol()` (2e-5 / 1.5e-2, absolute: probabilities are
<= 1).  The exact conditions (zero dK / dV rows of a fully hidden key, a hidden key's value never reaching O, hidden map
entries, bit-equality with the unmasked entries under an all-zeros mask, run-to-run bit-equality) are asserted with ==.

The mask is allocated wider than S (and its transpose wider than T) with NaN in the pad columns: whatever sits there must
never reach a result."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import ops  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402

DEV = "cuda"
B, H = 3, 2
SHAPES = [(5, 5, 32), (5, 5, 64), (64, 64, 32), (64, 64, 64), (65, 65, 32), (65, 65, 64), (130, 67, 32), (130, 67, 64),
          (65, 67, 96), (65, 67, 160)]
KINDS = ["finite", "holes", "mixed", "causal+finite"]
NINF = float("-inf")


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


def dead_column(S):
    return S // 3


def make_mask(kind, T, S):
    """fp32 [T, S] on the CPU; every row keeps a visible key by construction.  `holes` / `mixed`: column dead_column(S) is
    -inf in every row."""
    g = torch.Generator().manual_seed(1000 * T + S)
    finite = 2.0 * torch.randn(T, S, generator=g)
    if kind in ("finite", "causal+finite"):
        return finite
    holes = torch.zeros(T, S)
    holes[torch.rand(T, S, generator=g) < 0.4] = NINF
    rows = torch.arange(T)
    holes[rows, rows % S] = 0.0
    if S > 64:                                     # odd rows: the whole first key tile hidden (no visible key met yet)
        holes[1::2, :64] = NINF
        holes[1::2, 64] = 0.0
    dead = dead_column(S)
    holes[:, dead] = NINF
    # the dead column may have taken a row's guaranteed key (i % S == dead): give those rows another one
    for i in range(T):
        if torch.isinf(holes[i]).all():
            holes[i, (dead + 1) % S] = 0.0
    assert (~torch.isinf(holes)).any(dim=1).all()
    if kind == "holes":
        return holes
    return torch.where(torch.isinf(holes), holes, finite)          # "mixed"


def padded(m, extra):
    """[R, C] -> a device [R, ld] allocation, ld = C rounded up to 4 plus `extra` (a multiple of 4), NaN in the pad."""
    R, Cn = m.shape
    ld = (Cn + 3) // 4 * 4 + extra
    buf = torch.full((R, ld), float("nan"))
    buf[:, :Cn] = m
    return buf.to(DEV), ld


def device_mask(m):
    md, ldm = padded(m, 4)
    mt, ldt = padded(m.t().contiguous(), 8)
    return ops.attn_amasks([(md, ldm, mt, ldt)]), (md, mt)        # keep the tensors alive beside the descriptors


def dhp_for(dh):
    return 32 if dh <= 32 else 64 if dh <= 64 else 128 if dh <= 128 else 256


def setup(dtype, T, S, dh):
    dhp = dhp_for(dh)
    ctt = ops.ct_torch(dtype)
    d = H * dh
    ld = pad32(d)

    def heads(x):        # [B,H,L,dh] cpu -> device CT [B,H,L,dhp], and the CT-rounded values
        buf = torch.zeros(*x.shape[:3], dhp, dtype=ctt)
        buf[..., :dh] = x.to(ctt)
        return buf.to(DEV), buf[..., :dh].double()

    Q, q = heads(rnd(B, H, T, dh, seed=21) * dh ** -0.5)
    K, k = heads(rnd(B, H, S, dh, seed=22))
    V, v = heads(rnd(B, H, S, dh, seed=23))
    dO, do = heads(rnd(B, H, T, dh, seed=24))
    return dict(dhp=dhp, ctt=ctt, d=d, ld=ld, Q=Q, K=K, V=V, dO=dO, q=q, k=k, v=v, do=do)


def run(dtype, s, T, S, dh, off, am, pdrop=0.0, seed=9, maps=False):
    """Forward + both backward halves; am None = the unmasked entries.  Returns O, lse, dQ, dK, dV (device) [, W]."""
    ld, ctt = s["ld"], s["ctt"]
    O = torch.zeros(T * B, ld, device=DEV, dtype=ctt)
    lse, delta = torch.zeros(B, H, T, device=DEV), torch.zeros(B, H, T, device=DEV)
    dQ, dK, dV = (torch.full((L * B, ld), 7.0, device=DEV, dtype=ctt) for L in (T, S, S))
    p = ops.attn_problem(s["Q"], s["K"], s["V"], O, ld, lse, B, H, T, S, dh, s["dhp"], off, dO=s["dO"], delta=delta, dQ=dQ, lddq=ld,
                         dK=dK, lddk=ld, dV=dV, lddv=ld, dq_scale=1.0, drop_p=pdrop, drop_site=3)
    if am is None:
        ops.attn_fwd(dtype, [p], seed=seed)
        ops.attn_bwd_dq(dtype, [p], seed=seed)
        ops.attn_bwd_dkv(dtype, [p], seed=seed)
    else:
        ops.attn_fwd_amask(dtype, [p], am[0], seed=seed)
        ops.attn_bwd_dq_amask(dtype, [p], am[0], seed=seed)
        ops.attn_bwd_dkv_amask(dtype, [p], am[0], seed=seed)
    out = (O, lse, dQ, dK, dV)
    if maps:
        W = torch.full((B, T, S + 3), 5.0, device=DEV)
        mp = ops.attn_map_problem(s["Q"], s["K"], lse, W, S + 3, B, H, T, S, dh, s["dhp"], off)
        ops.attn_maps_amask(dtype, [mp], am[0])
        out += (W,)
    torch.cuda.synchronize()
    return out


_REF = {}


def reference(dtype, T, S, dh, kind):
    """fp64 restatement on the CT-rounded inputs, computed once per case."""
    key = (dtype, T, S, dh, kind)
    if key not in _REF:
        s = setup(dtype, T, S, dh)
        mask = make_mask(kind, T, S)
        off = 1 + abs(S - T) if kind == "causal+finite" else 0
        q, k, v = (s[n].clone().requires_grad_(True) for n in ("q", "k", "v"))
        sc = q @ k.transpose(-1, -2) + mask.double()[None, None]
        if off > 0:
            sc = sc.masked_fill(((torch.arange(S)[None, :] - torch.arange(T)[:, None]) >= off)[None, None], NINF)
        pr = torch.softmax(sc, -1)
        o_ref, lse_ref = pr @ v, torch.logsumexp(sc, -1)
        (o_ref * s["do"]).sum().backward()
        hidden = torch.isinf(sc.detach())[0, 0]                          # [T, S], the same in every head
        _REF[key] = (s, mask, off, o_ref.detach(), lse_ref.detach(), q.grad, k.grad, v.grad, pr.detach().mean(1), hidden)
    return _REF[key]


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh", SHAPES)
@pytest.mark.parametrize("kind", KINDS)
def test_additive_mask_attention_matches_fp64(dtype, T, S, dh, kind):
    s, mask, off, o_ref, lse_ref, dq_ref, dk_ref, dv_ref, w_ref, hidden = reference(dtype, T, S, dh, kind)
    am = device_mask(mask)
    O, lse, dQ, dK, dV, W = run(dtype, s, T, S, dh, off, am, maps=True)
    d = s["d"]

    def rows(x, L):      # row-major [(l*B+b), h*dh+c] -> [B,H,L,dh]
        return x[:, :d].float().reshape(L, B, H, dh).permute(1, 2, 0, 3)

    t = 3e-5 if dtype == BPM_F32 else 2e-2
    tb = 1e-4 if dtype == BPM_F32 else 4e-2
    close(rows(O, T), o_ref, t, "O")
    close(lse, lse_ref, t, "lse")
    close(rows(dQ, T), dq_ref, tb, "dQ")
    close(rows(dK, S), dk_ref, tb, "dK")
    close(rows(dV, S), dv_ref, tb, "dV")
    # head-averaged maps: tests/test_attn_maps_gpu.py's limits, hidden entries exact zeros, rows sum to 1
    tm = 2e-5 if dtype == BPM_F32 else 1.5e-2
    Wc = W.cpu()
    assert (Wc[:, :, S:] == 5.0).all(), "the maps kernel wrote past column S"
    w = Wc[:, :, :S]
    assert torch.isfinite(w).all()
    err = (w.double() - w_ref).abs().max().item()
    print(f"maps: max err {err:.3e} (limit {tm:.1e})")
    assert err <= tm, f"maps: max err {err:.3e} > {tm:.1e}"
    assert (w[hidden[None].expand(B, T, S)] == 0).all(), "a hidden map entry must be exactly 0.0f"
    rs = (w.double().sum(-1) - 1.0).abs().max().item()
    assert rs <= tm, f"maps: row sums off by {rs:.3e}"
    if kind in ("holes", "mixed"):
        dead = dead_column(S)
        # a key no query sees: exactly zero dK / dV rows
        dk4, dv4 = rows(dK, S).cpu(), rows(dV, S).cpu()                 # [B,H,S,dh]
        assert (dk4[:, :, dead] == 0).all() and (dv4[:, :, dead] == 0).all(), "dK / dV rows of a hidden key must be exact zeros"
        # its probability is exactly 0 in every row: moving its VALUE changes nothing, bit for bit
        s2 = dict(s)
        V2 = s["V"].clone()
        V2[:, :, dead] = 1000.0
        s2["V"] = V2
        O2 = run(dtype, s2, T, S, dh, off, am)[0]
        assert torch.equal(O2, O), "a hidden key's value row leaked into the output"


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh", [(65, 65, 64), (130, 132, 32), (65, 68, 160)])
@pytest.mark.parametrize("causal", [False, True])
@pytest.mark.parametrize("pdrop", [0.0, 0.1])
def test_all_zeros_mask_is_bit_equal_to_the_unmasked_entries(dtype, T, S, dh, causal, pdrop):
    """Same inputs, same seed: O, LSE, dQ, dK, dV of the *_amask entries under an all-zeros mask equal the unmasked entries'
    bit for bit -- with and without dropout on the probabilities (the element indexing of the dropout hash is the same;
    S % 4 == 0 takes the one-hash-per-four-keys path), with and without the mask_off rule."""
    s = setup(dtype, T, S, dh)
    off = 1 + abs(S - T) if causal else 0
    am = device_mask(torch.zeros(T, S))
    a = run(dtype, s, T, S, dh, off, None, pdrop)
    b = run(dtype, s, T, S, dh, off, am, pdrop)
    for x, y, nm in zip(a, b, ("O", "lse", "dQ", "dK", "dV")):
        assert torch.equal(x, y), f"{nm} differs from the unmasked entry"


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
def test_same_seed_twice_is_bit_equal_another_seed_differs(dtype):
    T, S, dh = 130, 67, 64
    s = setup(dtype, T, S, dh)
    am = device_mask(make_mask("mixed", T, S))
    a = run(dtype, s, T, S, dh, 0, am, 0.1)
    b = run(dtype, s, T, S, dh, 0, am, 0.1)
    for x, y, nm in zip(a, b, ("O", "lse", "dQ", "dK", "dV")):
        assert torch.equal(x, y), nm
        assert torch.isfinite(x.float()).all(), nm
    c = run(dtype, s, T, S, dh, 0, am, 0.1, seed=10)
    assert not torch.equal(c[0], a[0]), "another seed must draw another dropout mask"
