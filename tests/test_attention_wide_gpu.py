"""The attention kernels at padded head_dim 256 (any head_dim in (128, 256]), both compute types, against fp64 torch:
forward / dQ / dK-dV, the dQ pass's dS / Pd export with bpm_expand_heads, a group of problems with different lengths and
gathered query rows.  Same limits as the head_dim <= 128 tests of test_kernels_gpu.py."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import ops  # noqa: E402
from bpmult_amd.engine import dhp_for  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402
from test_kernels_gpu import attn_ref, close, drop_mult, rnd  # noqa: E402

DEV = "cuda"
DT = [BPM_F32, BPM_BF16]
WIDE = [136, 192, 256]


def heads(x, dh, dtype):
    """[B,H,L,dh] cpu -> device CT [B,H,L,dhp] zero padded, and the CT-rounded values (fp64)."""
    ctt = ops.ct_torch(dtype)
    buf = torch.zeros(*x.shape[:3], dhp_for(dh), dtype=ctt)
    buf[..., :dh] = x.to(ctt)
    return buf.to(DEV), buf[..., :dh].double()


class Case:
    """One attention problem: operands on the device, fp64 autograd reference, output buffers."""

    def __init__(self, dtype, B, H, T, S, dh, masked, pdrop, seed, site, qpos=None):
        ctt = ops.ct_torch(dtype)
        self.B, self.H, self.T, self.S, self.dh = B, H, T, S, dh
        self.d, self.ld = H * dh, pad32(H * dh)
        self.Q, q = heads(rnd(B, H, T, dh, seed=seed) * dh ** -0.5, dh, dtype)
        self.K, k = heads(rnd(B, H, S, dh, seed=seed + 1), dh, dtype)
        self.V, v = heads(rnd(B, H, S, dh, seed=seed + 2), dh, dtype)
        self.dO, do = heads(rnd(B, H, T, dh, seed=seed + 3), dh, dtype)
        q.requires_grad_(True); k.requires_grad_(True); v.requires_grad_(True)
        pm = drop_mult((B, H, T, S), pdrop, 9, site).double()
        if qpos is None:
            off = 1 + abs(S - T) if masked else 0
            o_ref, lse_ref = attn_ref(q, k, v, off, pm)
            pos = {}
        else:                                            # query row i at time step qpos0 + i * qstride of a T_full = S sequence
            off, (pos0, stride) = 1, qpos
            tpos = pos0 + stride * torch.arange(T)
            sc = (q @ k.transpose(-1, -2)).masked_fill((torch.arange(S)[None, :] - tpos[:, None]) >= off, float("-inf"))
            o_ref, lse_ref = (torch.softmax(sc, -1) * pm) @ v, torch.logsumexp(sc, -1)
            pos = dict(q_pos0=pos0, q_stride=stride)
        (o_ref * do).sum().backward()
        self.ref = dict(O=o_ref.detach(), lse=lse_ref.detach(), dQ=q.grad, dK=k.grad, dV=v.grad)
        self.O = torch.zeros(T * B, self.ld, device=DEV, dtype=ctt)
        self.lse, self.delta = torch.zeros(B, H, T, device=DEV), torch.zeros(B, H, T, device=DEV)
        self.dQ, self.dK, self.dV = (torch.zeros(L * B, self.ld, device=DEV, dtype=ctt) for L in (T, S, S))
        self.p = ops.attn_problem(self.Q, self.K, self.V, self.O, self.ld, self.lse, B, H, T, S, dh, dhp_for(dh), off, dO=self.dO,
                                  delta=self.delta, dQ=self.dQ, lddq=self.ld, dK=self.dK, lddk=self.ld, dV=self.dV, lddv=self.ld,
                                  dq_scale=1.0, drop_p=pdrop, drop_site=site, **pos)

    def rows(self, x, L):      # row-major [(l*B+b), h*dh+c] -> [B,H,L,dh]
        return x[:, :self.d].float().reshape(L, self.B, self.H, self.dh).permute(1, 2, 0, 3)

    def check(self, dtype, what=""):
        t = 3e-5 if dtype == BPM_F32 else 2e-2
        tb = 1e-4 if dtype == BPM_F32 else 4e-2
        close(self.rows(self.O, self.T), self.ref["O"], t, what + "O")
        close(self.lse, self.ref["lse"], t, what + "lse")
        assert (self.O[:, self.d:].float() == 0).all()
        close(self.rows(self.dQ, self.T), self.ref["dQ"], tb, what + "dQ")
        close(self.rows(self.dK, self.S), self.ref["dK"], tb, what + "dK")
        close(self.rows(self.dV, self.S), self.ref["dV"], tb, what + "dV")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh", WIDE)
@pytest.mark.parametrize("B,H,T,S,masked,pdrop", [(1, 2, 512, 200, True, 0.0),      # T > S
                                                   (1, 2, 200, 512, True, 0.0),      # T < S (band)
                                                   (1, 1, 513, 512, True, 0.0),      # T = S + 1
                                                   (2, 1, 1, 70, True, 0.0),         # a single query row
                                                   (1, 2, 130, 97, False, 0.0),      # no mask
                                                   (1, 2, 200, 512, True, 0.1)])     # attention dropout
def test_attention_fwd_bwd_wide(dtype, dh, B, H, T, S, masked, pdrop):
    c = Case(dtype, B, H, T, S, dh, masked, pdrop, seed=21, site=3)
    ops.attn_fwd(dtype, [c.p], seed=9)
    ops.attn_bwd(dtype, [c.p], seed=9)
    c.check(dtype)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh", WIDE)
def test_attention_group_of_six_wide(dtype, dh):
    """Six problems with different T / S (one masked with dropout, one unmasked) in one launch of each kernel."""
    shapes = [(2, 1, 70, 100, True, 0.0), (1, 2, 130, 130, True, 0.1), (1, 1, 100, 70, True, 0.0),
              (1, 1, 33, 65, False, 0.0), (2, 1, 2, 200, True, 0.0), (1, 1, 257, 64, True, 0.0)]
    cs = [Case(dtype, B, H, T, S, dh, m, p, seed=40 + 5 * i, site=3 + i) for i, (B, H, T, S, m, p) in enumerate(shapes)]
    ops.attn_fwd(dtype, [c.p for c in cs], seed=9)
    ops.attn_bwd(dtype, [c.p for c in cs], seed=9)
    for i, c in enumerate(cs):
        c.check(dtype, f"problem {i} ")


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh", WIDE)
def test_attention_gathered_query_rows_wide(dtype, dh):
    """q_pos0 / q_stride: query rows {0, S-1} of a T_full = S sequence against the reference at those positions."""
    S = 150
    c = Case(dtype, 2, 2, 2, S, dh, True, 0.0, seed=61, site=3, qpos=(0, S - 1))
    ops.attn_fwd(dtype, [c.p], seed=9)
    ops.attn_bwd(dtype, [c.p], seed=9)
    c.check(dtype)


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("dh", WIDE)
@pytest.mark.parametrize("B,H,T,S,pdrop,qpos", [(2, 2, 2, 200, 0.0, (0, 199)), (2, 2, 4, 132, 0.1, (0, 1)), (1, 2, 2, 512, 0.1, (0, 511))])
def test_attention_dq_pass_exports_dS_and_Pd_wide(dtype, dh, B, H, T, S, pdrop, qpos):
    """bpm_attn_bwd_dq with dS / Pd (the low-rank key side's factors) in the engine's [h*T + t][b][padded keys] layout, then
    bpm_expand_heads on the same operands, against fp64 torch."""
    ctt = ops.ct_torch(dtype)
    dhp = dhp_for(dh)
    d, ld, Sp = H * dh, pad32(H * dh), (S + 63) // 64 * 64
    Q, q = heads(rnd(B, H, T, dh, seed=31) * dh ** -0.5, dh, dtype)
    K, k = heads(rnd(B, H, S, dh, seed=32), dh, dtype)
    V, v = heads(rnd(B, H, S, dh, seed=33), dh, dtype)
    dO, do = heads(rnd(B, H, T, dh, seed=34), dh, dtype)
    pos0, stride = qpos[0], (qpos[1] - qpos[0]) if T == 2 else 1
    off = 1
    pm = drop_mult((B, H, T, S), pdrop, 9, 3).double()
    tpos = pos0 + stride * torch.arange(T)
    sc = (q @ k.transpose(-1, -2)).masked_fill((torch.arange(S)[None, :] - tpos[:, None]) >= off, float("-inf"))
    pr = torch.softmax(sc, -1)
    pd_ref = pr * pm
    o = pd_ref @ v
    ds_ref = pr * (pm * (do @ v.transpose(-1, -2)) - (do * o).sum(-1, keepdim=True))

    O = torch.zeros(T * B, ld, device=DEV, dtype=ctt)
    lse, delta = torch.zeros(B, H, T, device=DEV), torch.zeros(B, H, T, device=DEV)
    dQ = torch.zeros(T * B, ld, device=DEV, dtype=ctt)
    dS = torch.full((H * T, B, Sp), 7.0, device=DEV, dtype=ctt)
    Pd = torch.full((H * T, B, Sp), 7.0, device=DEV, dtype=ctt)
    p = ops.attn_problem(Q, K, V, O, ld, lse, B, H, T, S, dh, dhp, off, dO=dO, delta=delta, dQ=dQ, lddq=ld, dq_scale=1.0,
                         drop_p=pdrop, drop_site=3, q_pos0=pos0, q_stride=stride, dS=dS, Pd=Pd, xs=(Sp, T * B * Sp, B * Sp))
    ops.attn_fwd(dtype, [p], seed=9)
    ops.attn_bwd_dq(dtype, [p], seed=9)
    torch.cuda.synchronize()
    t = 1e-4 if dtype == BPM_F32 else 3e-2
    got_ds = dS.float().reshape(H, T, B, Sp).permute(2, 0, 1, 3)
    got_pd = Pd.float().reshape(H, T, B, Sp).permute(2, 0, 1, 3)
    # keys beyond the last visible one of the block's last query are never visited (the dQ key tile is 32 at dhp 256)
    vis = int(min(S, tpos.max().item() + off))
    nt = min((vis + 31) // 32 * 32, S)
    # bf16 dS = P (dP - delta) with delta = rowsum(dO * O) from the bf16-ROUNDED O the forward stored: a single visible key
    # gives dS = 0 exactly but leaves |dP| * 2^-9 of rounding, which grows as sqrt(head_dim) (measured 3.1e-2 at head_dim 136,
    # S = 512, dropout 0.1): held to the 4e-2 gradient limit of the dQ / dK / dV checks instead of 3e-2
    close(got_ds[..., :nt], ds_ref[..., :nt], t if dtype == BPM_F32 else 4e-2, "dS")
    close(got_pd[..., :nt], pd_ref[..., :nt], t, "Pd")
    assert (got_ds[..., S:] == 7.0).all() and (got_pd[..., S:] == 7.0).all(), "key padding must not be written"
    q_dq = q.detach().clone().requires_grad_(True)
    sc2 = (q_dq @ k.transpose(-1, -2)).masked_fill((torch.arange(S)[None, :] - tpos[:, None]) >= off, float("-inf"))
    ((torch.softmax(sc2, -1) * pm) @ v * do).sum().backward()
    close(dQ[:, :d].float().reshape(T, B, H, dh).permute(1, 2, 0, 3), q_dq.grad, 1e-4 if dtype == BPM_F32 else 4e-2, "dQ")
    # ---- expand_heads at this head_dim
    qexp = torch.full((H * T * B, ld), 5.0, device=DEV, dtype=ctt)
    doexp = torch.full((H * T * B, ld), 5.0, device=DEV, dtype=ctt)
    dbias = torch.full((d,), 3.0, device=DEV)
    Pz = Pd.clone()
    Pz[..., S:] = 0
    ops.expand_heads(dtype, [ops.expand_problem(Q, dO, qexp, doexp, B, H, T, dh, dhp, ld, Pd=Pz, S=Sp, dbias=dbias)])
    torch.cuda.synchronize()
    ref_q = torch.zeros(H, T, B, ld, dtype=torch.float64)
    ref_do = torch.zeros(H, T, B, ld, dtype=torch.float64)
    for h in range(H):
        ref_q[h, :, :, h * dh:(h + 1) * dh] = q.detach()[:, h].permute(1, 0, 2)
        ref_do[h, :, :, h * dh:(h + 1) * dh] = do[:, h].permute(1, 0, 2)
    assert torch.equal(qexp.float().cpu().double().reshape(H, T, B, ld), ref_q)
    assert torch.equal(doexp.float().cpu().double().reshape(H, T, B, ld), ref_do)
    rs = Pz.float().cpu().double().reshape(H, T, B, Sp).sum(-1)
    ref_b = torch.einsum("htb,bhtj->hj", rs, do).reshape(d)
    close(dbias, ref_b, 1e-5 if dtype == BPM_F32 else 1e-3, "value-bias gradient")
