"""Attention with a per-key padding mask (bpm_attn_fwd_kmask / _bwd_dq_kmask / _bwd_dkv_kmask) on the MI355X against an
fp64 torch restatement: additive -inf on hidden keys, softmax, P V, autograd for dQ / dK / dV.  Tolerances are the ones
tests/test_kernels_gpu.py::test_attention_fwd_bwd applies to the unmasked entries (forward 3e-5 / 2e-2, backward
1e-4 / 4e-2 for f32 / bf16, relative to max(1, |ref|max)); the exact conditions (zero rows of hidden keys, bit-equality
with the unmasked entries under an all-ones mask, run-to-run bit-equality) are asserted with ==."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import ops  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402

DEV = "cuda"
B, H = 3, 2
SHAPES = [(5, 5), (64, 64), (65, 65), (130, 67)]


def rnd(*shape, seed):
    return torch.randn(*shape, generator=torch.Generator().manual_seed(seed))


def close(got, ref, t, what):
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape, (what, got.shape, ref.shape)
    assert torch.isfinite(got).all(), what + ": non-finite"
    scale = max(1.0, ref.abs().max().item())
    err = (got - ref).abs().max().item()
    assert err <= t * scale, f"{what}: max err {err:.3e} vs tol {t * scale:.3e}"


def make_mask(kind, S):
    """uint8 [B, S], tight (ldm = S).  Every sample keeps at least one visible key."""
    m = torch.zeros(B, S, dtype=torch.uint8)
    if kind == "prefix":                       # lengths 1, S - 1, S
        lens = [1, max(1, S - 1), S]
    elif kind == "offtile":                    # lengths that are no multiple of the 64-key tile (nor of 32, nor of 4)
        lens = [min(3, S), max(1, S - 2), (S + 1) // 2]
    else:
        lens = None
    if lens is not None:
        for b, n in enumerate(lens):
            m[b, :n] = 1
        return m
    g = torch.Generator().manual_seed(100 + S)
    m = (torch.rand(B, S, generator=g) > 0.4).to(torch.uint8)
    if kind == "holes":
        m[0, 0] = 0                            # sample 0: the first key hidden
        m[0, S - 1] = 1
        if S > 64:
            m[1, :64] = 0                      # sample 1: the whole first key tile hidden (no visible key met yet)
            m[1, 64] = 1
        else:
            m[1, S - 1] = 1
        m[2, S // 2] = 1
    else:                                      # "causal": combined with mask_off, every query must keep a visible key
        m[:, 0] = 1
    return m


def setup(dtype, T, S, dh):
    dhp = 32 if dh <= 32 else 64
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


def run(dtype, s, T, S, dh, off, mask_dev, pdrop=0.0, seed=9):
    """Forward + both backward halves; mask_dev None = the unmasked entries.  Returns O, lse, dQ, dK, dV (device)."""
    ld, ctt = s["ld"], s["ctt"]
    O = torch.zeros(T * B, ld, device=DEV, dtype=ctt)
    lse, delta = torch.zeros(B, H, T, device=DEV), torch.zeros(B, H, T, device=DEV)
    dQ, dK, dV = (torch.full((L * B, ld), 7.0, device=DEV, dtype=ctt) for L in (T, S, S))
    p = ops.attn_problem(s["Q"], s["K"], s["V"], O, ld, lse, B, H, T, S, dh, s["dhp"], off, dO=s["dO"], delta=delta, dQ=dQ, lddq=ld,
                         dK=dK, lddk=ld, dV=dV, lddv=ld, dq_scale=1.0, drop_p=pdrop, drop_site=3)
    if mask_dev is None:
        ops.attn_fwd(dtype, [p], seed=seed)
        ops.attn_bwd_dq(dtype, [p], seed=seed)
        ops.attn_bwd_dkv(dtype, [p], seed=seed)
    else:
        km = ops.attn_kmasks([(mask_dev, S)])
        ops.attn_fwd_kmask(dtype, [p], km, seed=seed)
        ops.attn_bwd_dq_kmask(dtype, [p], km, seed=seed)
        ops.attn_bwd_dkv_kmask(dtype, [p], km, seed=seed)
    torch.cuda.synchronize()
    return O, lse, dQ, dK, dV


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("dh", [32, 64])
@pytest.mark.parametrize("T,S", SHAPES)
@pytest.mark.parametrize("kind", ["prefix", "offtile", "holes", "causal"])
def test_key_masked_attention_matches_fp64(dtype, dh, T, S, kind):
    s = setup(dtype, T, S, dh)
    mask = make_mask(kind, S)
    assert mask.is_contiguous() and mask.shape == (B, S)            # ldm = S exactly; S is odd in three of the four shapes
    off = 1 + abs(S - T) if kind == "causal" else 0
    q, k, v, do = (s[n].clone().requires_grad_(n != "do") for n in ("q", "k", "v", "do"))
    sc = q @ k.transpose(-1, -2)
    hidden = (mask == 0)[:, None, None, :].expand(B, H, T, S).clone()
    if off > 0:
        hidden |= ((torch.arange(S)[None, :] - torch.arange(T)[:, None]) >= off)[None, None]
    sc = sc.masked_fill(hidden, float("-inf"))
    pr = torch.softmax(sc, -1)
    o_ref, lse_ref = pr @ v, torch.logsumexp(sc, -1)
    (o_ref * do).sum().backward()

    O, lse, dQ, dK, dV = run(dtype, s, T, S, dh, off, mask.to(DEV))
    d = s["d"]

    def rows(x, L):      # row-major [(l*B+b), h*dh+c] -> [B,H,L,dh]
        return x[:, :d].float().reshape(L, B, H, dh).permute(1, 2, 0, 3)

    t = 3e-5 if dtype == BPM_F32 else 2e-2
    tb = 1e-4 if dtype == BPM_F32 else 4e-2
    close(rows(O, T), o_ref.detach(), t, "O")
    close(lse, lse_ref.detach(), t, "lse")
    close(rows(dQ, T), q.grad, tb, "dQ")
    close(rows(dK, S), k.grad, tb, "dK")
    close(rows(dV, S), v.grad, tb, "dV")
    # hidden keys: exactly zero dK / dV rows
    gone = (mask == 0)                                              # [B, S]
    dk4, dv4 = rows(dK, S).cpu(), rows(dV, S).cpu()                 # [B,H,S,dh]
    sel = gone[:, None, :, None].expand_as(dk4)
    assert (dk4[sel] == 0).all() and (dv4[sel] == 0).all(), "dK / dV rows of hidden keys must be exact zeros"
    # the probabilities of hidden keys are exactly 0: moving their VALUES changes nothing, bit for bit
    s2 = dict(s)
    V2 = s["V"].clone()
    V2[gone.to(DEV)[:, None, :].expand(B, H, S)] = 1000.0
    s2["V"] = V2
    O2 = run(dtype, s2, T, S, dh, off, mask.to(DEV))[0]
    assert torch.equal(O2, O), "a hidden key's value row leaked into the output"


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("T,S,dh,causal,pdrop", [(65, 65, 64, False, 0.0), (65, 65, 64, False, 0.1), (130, 67, 32, False, 0.1),
                                                 (130, 67, 64, True, 0.0), (64, 64, 32, True, 0.1), (5, 5, 64, False, 0.1),
                                                 (130, 132, 64, False, 0.1)])
def test_all_ones_mask_is_bit_equal_to_the_unmasked_entries(dtype, T, S, dh, causal, pdrop):
    """Same inputs, same seed: outputs, LSE, dQ, dK, dV of the *_kmask entries under an all-ones mask equal the unmasked
    entries' bit for bit -- also with dropout on the probabilities (the element indexing of the dropout hash is the same;
    S % 4 == 0 takes the one-hash-per-four-keys path)."""
    s = setup(dtype, T, S, dh)
    off = 1 + abs(S - T) if causal else 0
    ones = torch.ones(B, S, dtype=torch.uint8, device=DEV)
    a = run(dtype, s, T, S, dh, off, None, pdrop)
    b = run(dtype, s, T, S, dh, off, ones, pdrop)
    for x, y, nm in zip(a, b, ("O", "lse", "dQ", "dK", "dV")):
        assert torch.equal(x, y), f"{nm} differs from the unmasked entry"
    if pdrop > 0:
        c = run(dtype, s, T, S, dh, off, ones, pdrop, seed=10)
        assert not torch.equal(c[0], b[0]), "another seed must draw another dropout mask"


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
def test_same_seed_twice_is_bit_equal(dtype):
    T, S, dh = 130, 67, 64
    s = setup(dtype, T, S, dh)
    mask = make_mask("holes", S).to(DEV)
    a = run(dtype, s, T, S, dh, 0, mask, 0.1)
    b = run(dtype, s, T, S, dh, 0, mask, 0.1)
    for x, y, nm in zip(a, b, ("O", "lse", "dQ", "dK", "dV")):
        assert torch.equal(x, y), nm
    assert torch.isfinite(a[0].float()).all() and torch.isfinite(a[2].float()).all()
