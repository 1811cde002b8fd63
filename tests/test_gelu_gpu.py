"""Exact (erf) GELU row kernels (bpm_gelu_fwd / bpm_gelu_bwd) on the MI355X against torch fp64 gelu(approximate="none").

Error measure for fp32 values: max |got - ref| / max(1, |ref|) -- relative for large values, absolute below 1 (a purely
relative measure would be meaningless for torch's own result on the negative tail: 1 + erf cancels completely in fp32 at
u = -6, where bpm_gelu uses erfc and keeps full precision).  Tolerance: what torch's OWN fp32 GELU (forward and autograd
backward, same device, same inputs) shows in that measure against the fp64 value, times 2 -- measured inside the test --
with a floor of "a few ulp" (4 * 2^-24) where torch happens to be exact.
CT (bf16) outputs: per ELEMENT, |got - ref| <= |ref| * 2^-8 + the fp32 tolerance * max(1, |ref|).  2^-8 is one
round-to-nearest bf16 rounding: bf16 keeps 8 significant bits, so values in [2^e, 2^(e+1)) are 2^(e-7) apart and the
nearest one is at most 2^(e-8) <= |ref| * 2^-8 away (the bound is met with equality just above a power of two).
The saturated tails are checked by value below."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import ops  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402

DEV = "cuda"
SPECIAL = [0.0, 1e-4, -1e-4, 6.0, -6.0, 30.0, -30.0, 1.0, -1.0, 3.0, -3.0, 0.5, -0.5, 10.0, -10.0]
ULP = 2.0 ** -24


def inputs(R, N, seed):
    g = torch.Generator().manual_seed(seed)
    u = torch.randn(R, N, generator=g) * 2.0
    u.view(-1)[:len(SPECIAL)] = torch.tensor(SPECIAL)
    u[-1, -len(SPECIAL):] = torch.tensor(SPECIAL)             # also in the last row's last chunks
    dg = torch.randn(R, N, generator=g)
    return u, dg


def ref64(u, dg):
    x = u.double().requires_grad_(True)
    y = torch.nn.functional.gelu(x, approximate="none")
    (y * dg.double()).sum().backward()
    return y.detach(), x.grad


def rel_err(got, ref):
    """max |got - ref| / max(1, |ref|)"""
    return ((got.double() - ref).abs() / ref.abs().clamp_min(1.0)).max().item()


def torch_f32_error(u, dg, y_ref, du_ref):
    """what torch's fp32 GELU achieves on the device: (relative forward error, relative backward error)"""
    x = u.to(DEV).requires_grad_(True)
    y = torch.nn.functional.gelu(x, approximate="none")
    (y * dg.to(DEV)).sum().backward()
    return rel_err(y.detach().cpu(), y_ref), rel_err(x.grad.cpu(), du_ref)


@pytest.mark.parametrize("dtype", [BPM_F32, BPM_BF16])
@pytest.mark.parametrize("u_is_ct", [False, True])
@pytest.mark.parametrize("R,N", [(3, 70), (257, 3072)])
def test_gelu_fwd_bwd(dtype, u_is_ct, R, N):
    N_k = N
    ctt = ops.ct_torch(dtype)
    u, dg = inputs(R, N, seed=R + N)
    ld = pad32(N)
    # input rows: fp32 with the leading dimension rounded up to whole 4-element chunks (72 for N = 70), or CT [R, ld]
    if u_is_ct:
        ub = torch.zeros(R, ld, dtype=ctt)
        ub[:, :N] = u.to(ctt)
        u_used = ub[:, :N].float()
        u_dev, ldu = ub.to(DEV), ld
    else:
        ldu = (N + 3) // 4 * 4
        ub = torch.zeros(R, ldu)
        ub[:, :N] = u
        u_used, u_dev = u, ub.to(DEV)
    lddg = (N + 3) // 4 * 4
    dgb = torch.zeros(R, lddg)
    dgb[:, :N] = dg
    y_ref, du_ref = ref64(u_used[:, :N_k], dg[:, :N_k])
    e_f, e_b = torch_f32_error(u_used[:, :N_k], dg[:, :N_k], y_ref, du_ref)
    print(f"torch fp32 gelu on this device: rel fwd err {e_f:.3e}, rel bwd err {e_b:.3e}")
    tol_f, tol_b = 2 * max(e_f, 4 * ULP), 2 * max(e_b, 4 * ULP)
    rnd = 2.0 ** -8 if dtype == BPM_BF16 else 0.0          # one bf16 rounding of the element itself

    g = torch.full((R, ld), 7.0, device=DEV, dtype=ctt)
    du = torch.full((R, ld), 7.0, device=DEV, dtype=ctt)
    ops.gelu_fwd(dtype, [ops.gelu_problem(u_dev, ldu, R, N_k, u_is_ct=u_is_ct, g=g, ldg=ld)])
    ops.gelu_bwd(dtype, [ops.gelu_problem(u_dev, ldu, R, N_k, u_is_ct=u_is_ct, dg=dgb.to(DEV), lddg=lddg, du=du, lddu=ld)])
    torch.cuda.synchronize()
    gc, duc = g.float().cpu(), du.float().cpu()
    assert torch.isfinite(gc).all() and torch.isfinite(duc).all()
    assert (gc[:, N_k:] == 0).all() and (duc[:, N_k:] == 0).all(), "pad columns [N, ld) must be zero"
    def excess(got, ref, tol):          # max over elements of |got - ref| / (|ref| * rnd + tol * max(1, |ref|)): <= 1 passes
        return ((got.double() - ref).abs() / (ref.abs() * rnd + tol * ref.abs().clamp_min(1.0))).max().item()

    ef, eb = excess(gc[:, :N_k], y_ref, tol_f), excess(duc[:, :N_k], du_ref, tol_b)
    print(f"bpm_gelu: fwd err / bound {ef:.3f} (fp32 tol {tol_f:.3e}), bwd err / bound {eb:.3f} (fp32 tol {tol_b:.3e}), rounding {rnd:.3e}")
    assert ef <= 1.0, f"forward: error {ef:.3f} x the per-element bound"
    assert eb <= 1.0, f"backward: error {eb:.3f} x the per-element bound"
    # the named points, exactly where exactness is owed
    sp = torch.tensor(SPECIAL[:7])
    got = gc[0, :7]
    assert got[0] == 0 and got[5] == 30.0 and got[6] == 0, got          # gelu(0) = 0, gelu(30) = 30, gelu(-30) = -0
    assert (got[3] - 6.0).abs() <= 6.0 * 2.0 ** -7 and got[4] <= 0 and got[4] > -1e-7, got
    # gelu(-6) = -5.92e-9: the negative tail keeps its leading digits (torch's fp32 result is -0); bf16: one rounding of it
    assert abs(got[4].item() / ref64(sp, sp)[0][4].item() - 1) < (1e-3 if dtype == BPM_F32 else 2.0 ** -8 + 1e-3), got[4]


def test_gelu_groups_of_problems():
    """Several problems per launch (the row kernels' grouping): each problem's rows land in its own output."""
    dtype, ctt = BPM_BF16, torch.bfloat16
    shapes = [(3, 68), (70, 128), (1, 4)]
    probs, keep = [], []
    for i, (R, N) in enumerate(shapes):
        u = torch.randn(R, N, generator=torch.Generator().manual_seed(i)).to(DEV)
        g = torch.full((R, pad32(N)), 7.0, device=DEV, dtype=ctt)
        probs.append(ops.gelu_problem(u, N, R, N, g=g, ldg=pad32(N)))
        keep.append((u, g, N))
    ops.gelu_fwd(dtype, probs)
    torch.cuda.synchronize()
    for u, g, N in keep:
        ref = torch.nn.functional.gelu(u.double().cpu(), approximate="none")
        got = g[:, :N].float().cpu().double()
        assert ((got - ref).abs() <= ref.abs() * 2.0 ** -8 + 8 * ULP * ref.abs().clamp_min(1.0)).all()
        assert (g[:, N:].float() == 0).all()
