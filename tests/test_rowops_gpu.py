"""Row kernels (csrc/rows_pack.hip, rows_norm.hip, rows_elem.hip, adam.hip) at the sizes where they change regime, and the entry points no other kernel test
reaches: LayerNorm past its block caps and through the workspace hand-off, the column-sum kernel over many 128-row
blocks, interleaved CT output, add_n, zero_segments, split_rows, device tables with several descriptors, the
element-wise embed_pos path and the grid-stride caps of pack_rows / gmu2.

References are fp64 torch on the CPU; where the operation is exact in IEEE fp32 the reference is its fp32 restatement
and the comparison is bitwise.  Every output is a view into a larger sentinel-filled buffer whose bytes around the view
must come back unchanged, and every column-sum check first proves on the reference alone that one lost or doubled row
would be at least 10x the tolerance.

Each check was seen to fail under a wrong kernel (tried, not kept).  LayerNorm backward, vector kernel: `row + 1 < P.R`
for the live-row test (dx of the last row stays NaN: multi_block at d = 300 / 768 / 1024, all three ln_bwd_ws tests),
the last block's sum starting at b = 1 (dgamma / cast_colsum: multi_block, six_problems, absent_sums), no ticket reset
("ticket words left set"; later launches of multi_block lose their sums), cast_colsum adding the dbeta sums on the
atomics path (six_problems, shared_and_unaligned).  Scalar kernel: the second LDS pass reading the first pass's
registers (dbeta at d = 770 / 1028 / 1536, large_mean[770]).  Forward row loops with twice the stride (past_its_block_cap,
d = 24 vector, d = 50 scalar).  colsum_kernel dropping a block's last row (many_row_blocks); the general kernel skipping
the last column's sum (past_the_chunk_limit, interleaved) or writing ldd instead of ct_cols columns (interleaved: "right
half written").  add_n tail one thread short; zero_segments one element or one quad short; split_rows rounding
x * 1.0000001; `<` for `<=` in either binary search (descriptor 1 of pack_weights / fold_bias / unfold_grads,
zero_segments); unfold_grads ignoring store_dw; embed_pos without pos_stride, or with scale * mask folded first (bitwise
check against the vector path); pack_rows / gmu2 loops with a longer stride; a sigmoid written e / (1 + e) (NaN at +100).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import _lib, ops  # noqa: E402
from bpmult_amd.ops import BPM_BF16, BPM_F32, pad32  # noqa: E402
from test_kernels_gpu import DEV, DT, close, drop_mult, rnd, to_ct  # noqa: E402

NAN = float("nan")
CT_FILL = -24576.0            # sentinel of CT buffers: -1.5 * 2^14, exact in bf16 and f32


class Guarded:
    """An output tensor as a view into a larger buffer prefilled with a sentinel; check() asserts that the bytes in
    front of and behind the view are unchanged.  skew: elements by which the view is moved off 16-byte alignment."""
    G = 64

    def __init__(self, *shape, dtype=torch.float32, fill=NAN, skew=0, start=None):
        self.n = int(np.prod(shape))
        self.lo = self.G + skew
        self.buf = torch.full((self.lo + self.n + self.G,), fill, dtype=dtype, device=DEV)
        self.v = self.buf[self.lo:self.lo + self.n].view(*shape)
        if start is not None:
            self.v.copy_(start)
        self.init = self.buf.clone()

    def _bits(self, t):
        return t.view(torch.int16 if t.element_size() == 2 else torch.int32)

    def reset(self):
        self.buf.copy_(self.init)

    def check(self, what):
        got, was = self._bits(self.buf), self._bits(self.init)
        assert torch.equal(got[:self.lo], was[:self.lo]), what + ": bytes in front of the output were written"
        assert torch.equal(got[self.lo + self.n:], was[self.lo + self.n:]), what + ": bytes behind the output were written"


def ct_out(*shape, dtype):
    return Guarded(*shape, dtype=ops.ct_torch(dtype), fill=CT_FILL)


def bits(t):
    return t.contiguous().view(torch.int16 if t.element_size() == 2 else torch.int32)


def assert_sensitive(contrib, t, ref, what, skip=()):
    """contrib: fp64 [R, C] contribution of every row to a column sum whose reference is `ref` and whose tolerance is
    t * max(1, |ref|max) (close()): every row's largest contribution is at least ten times that, so the tolerance
    cannot hide one lost or doubled row."""
    bound = 10 * t * max(1.0, ref.double().abs().max().item())
    per_row = contrib.double().abs().amax(1)
    keep = torch.ones(per_row.numel(), dtype=torch.bool)
    for r in skip:
        keep[r] = False
    low = per_row[keep].min().item()
    assert low >= bound, f"{what}: smallest single-row contribution {low:.3e} < 10 x tolerance {bound:.3e}"


def ln_ref64(x, gamma, beta, dy, eps=1e-5):
    """fp64 LayerNorm (biased variance, eps inside the sqrt) and its backward: y, dx, mean, rstd, xhat."""
    x, gamma, dy = x.double(), gamma.double(), dy.double()
    mu = x.mean(1, keepdim=True)
    rs = (x.var(1, unbiased=False, keepdim=True) + eps).rsqrt()
    xh = (x - mu) * rs
    y = xh * gamma + (beta.double() if beta is not None else 0.0)
    g = dy * gamma
    dx = rs * (g - g.mean(1, keepdim=True) - xh * (g * xh).mean(1, keepdim=True))
    return y, dx, mu[:, 0], rs[:, 0], xh


# ---------------------------------------------------------------------------
# 1. LayerNorm at multi-block row counts
# ---------------------------------------------------------------------------
LN_R = 1037          # 2 * 512 + 13: the vector backward (64 blocks x 4 waves x 2 rows) makes a third, mostly idle
#                      iteration in which one wave holds a live and a dead row; the scalar backward (256 x 4) a second
LN_D = [300, 768, 1024, 1028, 50, 770, 1536]
LN_SEED, LN_SITE, LN_P = 1234, 9, 0.2
ZERO_ROW, CONST_ROW = 1, 2


@functools.lru_cache(maxsize=2)
def ln_case(R, d, with_bwd=True):
    """Inputs as in test_kernels_gpu.test_layernorm (x = 2 randn + 0.5, dy = randn, same seeds), the fp64 reference and
    the sensitivity of every column sum, computed once per shape and shared by both CT dtypes."""
    c = SimpleNamespace(R=R, d=d)
    c.x = rnd(R, d, seed=41) * 2 + 0.5
    c.x[ZERO_ROW] = 0.0                   # an all-zero (padded) row: LN(0) = beta
    c.x[CONST_ROW] = 0.5                  # a constant row: xhat = 0, rstd = eps^-1/2
    c.gamma = 1 + 0.1 * rnd(d, seed=42)
    c.beta = 0.1 * rnd(d, seed=43)
    c.dy = rnd(R, d, seed=44) if with_bwd else torch.zeros(R, d)
    c.y, dx, c.mean, c.rstd, xh = ln_ref64(c.x, c.gamma, c.beta, c.dy)
    if not with_bwd:
        return c
    c.add = rnd(R, d, seed=45)
    c.dx, c.dx_add = dx, dx + c.add.double()
    c.g0, c.b0, c.c0 = rnd(d, seed=46), rnd(d, seed=47), rnd(d, seed=48)      # the sums accumulate: non-zero start
    cg, cb = c.dy.double() * xh, c.dy.double()
    c.dgamma, c.dbeta = c.g0.double() + cg.sum(0), c.b0.double() + cb.sum(0)
    assert_sensitive(cg, 1e-4, c.dgamma, "dgamma", skip=(ZERO_ROW, CONST_ROW))   # constant rows: xhat = 0
    assert_sensitive(cb, 1e-4, c.dbeta, "dbeta")
    c.mult = drop_mult((R, d), LN_P, LN_SEED, LN_SITE)
    c.cast = c.dx_add * c.mult.double()
    c.csum = c.c0.double() + c.cast.sum(0)
    assert_sensitive(c.cast, 1e-4, c.csum, "cast_colsum")
    c.plain = torch.ones(R, dtype=torch.bool)
    c.plain[ZERO_ROW] = c.plain[CONST_ROW] = False
    return c


@pytest.mark.parametrize("d,dtype", [(d, dt) for d in LN_D for dt in DT])
def test_layernorm_multi_block(d, dtype):
    c, R, ld = ln_case(LN_R, d), LN_R, pad32(d)
    tf = 2e-5 if dtype == BPM_F32 else 1e-2
    xd, gd, bd, dyd, addd = (t.to(DEV) for t in (c.x, c.gamma, c.beta, c.dy, c.add))
    out, outf = ct_out(R, ld, dtype=dtype), Guarded(R, d)
    mean, rstd, mean2, rstd2 = (Guarded(R) for _ in range(4))
    ops.ln_fwd(dtype, [ops.ln_problem(xd, gd, bd, mean.v, rstd.v, R, out=out.v, ldo=ld),
                       ops.ln_problem(xd, gd, bd, mean2.v, rstd2.v, R, out=outf.v, ldo=d, out_f32=True)], d)
    close(out.v[:, :d].float(), c.y, tf, "ln fwd")
    assert (out.v[:, d:].float() == 0).all()
    close(outf.v, c.y, 2e-5, "ln fwd f32")
    close(mean.v, c.mean, 2e-5, "ln mean")
    close(rstd.v, c.rstd, 2e-5, "ln rstd")
    assert torch.equal(mean.v, mean2.v) and torch.equal(rstd.v, rstd2.v)
    for g, nm in ((out, "out"), (outf, "out f32"), (mean, "mean"), (rstd, "rstd"), (mean2, "mean 2"), (rstd2, "rstd 2")):
        g.check("ln fwd " + nm)

    dx, dx2 = Guarded(R, d), Guarded(R, d)
    dgam, dbet = Guarded(d, start=c.g0), Guarded(d, start=c.b0)
    ops.ln_bwd([ops.ln_problem(xd, gd, None, mean.v, rstd.v, R, dy=dyd, ldy=d, add=addd, dx=dx.v, dgamma=dgam.v, dbeta=dbet.v),
                ops.ln_problem(xd, gd, None, mean.v, rstd.v, R, dy=dyd, ldy=d, dx=dx2.v)], d)
    close(dx.v, c.dx_add, 1e-4, "ln dx")
    close(dx2.v, c.dx, 1e-4, "ln dx (no add, no param grads)")
    # the zero and the constant row have rstd = 316 and set the scale above: the ordinary rows on their own scale
    close(dx.v[c.plain.to(DEV)], c.dx_add[c.plain], 1e-4, "ln dx, ordinary rows")
    close(dx2.v[c.plain.to(DEV)], c.dx[c.plain], 1e-4, "ln dx (no add), ordinary rows")
    close(dgam.v, c.dgamma, 1e-4, "ln dgamma")
    close(dbet.v, c.dbeta, 1e-4, "ln dbeta")
    for g, nm in ((dx, "dx"), (dx2, "dx 2"), (dgam, "dgamma"), (dbet, "dbeta")):
        g.check("ln bwd " + nm)

    # fused hand-off: CT copy of dropmask(dx) with zero pad + its column sums
    dx3, cast, cs = Guarded(R, d), ct_out(R, ld, dtype=dtype), Guarded(d, start=c.c0)
    ops.ln_bwd([ops.ln_problem(xd, gd, None, mean.v, rstd.v, R, dy=dyd, ldy=d, add=addd, dx=dx3.v, cast=cast.v, ldc=ld,
                               cast_colsum=cs.v, drop_p=LN_P, drop_site=LN_SITE)], d, dtype, LN_SEED)
    assert torch.equal(dx3.v, dx.v)
    close(cast.v[:, :d].float(), dx.v.cpu() * c.mult, 1e-6 if dtype == BPM_F32 else 1e-2, "ln fused cast against dx")
    close(cast.v[:, :d].float(), c.cast, 1e-4 if dtype == BPM_F32 else 1e-2, "ln fused cast")
    assert (cast.v[:, d:].float() == 0).all()
    close(cs.v, c.csum, 1e-4, "ln fused colsum")
    for g, nm in ((dx3, "dx"), (cast, "cast"), (cs, "cast_colsum")):
        g.check("ln fused " + nm)


@pytest.mark.parametrize("d,dtype", [(d, dt) for d in (24, 50) for dt in DT])
def test_layernorm_forward_past_its_block_cap(d, dtype):
    """R = 16390 rows: 4096 blocks x 4 waves cover 16384, so the forward's row loop iterates (vector kernel at d = 24,
    scalar at d = 50)."""
    R, ld = 16390, pad32(d)
    c = ln_case(R, d, False)
    xd, gd, bd = (t.to(DEV) for t in (c.x, c.gamma, c.beta))
    out, outf = ct_out(R, ld, dtype=dtype), Guarded(R, d)
    mean, rstd, mean2, rstd2 = (Guarded(R) for _ in range(4))
    ops.ln_fwd(dtype, [ops.ln_problem(xd, gd, bd, mean.v, rstd.v, R, out=out.v, ldo=ld),
                       ops.ln_problem(xd, gd, bd, mean2.v, rstd2.v, R, out=outf.v, ldo=d, out_f32=True)], d)
    close(out.v[:, :d].float(), c.y, 2e-5 if dtype == BPM_F32 else 1e-2, "ln fwd")
    assert (out.v[:, d:].float() == 0).all()
    close(outf.v, c.y, 2e-5, "ln fwd f32")
    close(mean.v, c.mean, 2e-5, "ln mean")
    close(rstd.v, c.rstd, 2e-5, "ln rstd")
    close(mean2.v, c.mean, 2e-5, "ln mean 2")
    close(rstd2.v, c.rstd, 2e-5, "ln rstd 2")
    for g, nm in ((out, "out"), (outf, "out f32"), (mean, "mean"), (rstd, "rstd"), (mean2, "mean 2"), (rstd2, "rstd 2")):
        g.check("ln fwd " + nm)


def close_or(got, ref, t, floor, what):
    """close() with the bound max(t * max(1, |ref|max), floor)."""
    got, ref = got.detach().cpu().double(), ref.double()
    assert got.shape == ref.shape and torch.isfinite(got).all(), what
    err = (got - ref).abs().max().item()
    bound = max(t * max(1.0, ref.abs().max().item()), floor)
    print(f"{what}: max err {err:.3e}, bound {bound:.3e}")
    assert err <= bound, f"{what}: max err {err:.3e} vs bound {bound:.3e}"


@pytest.mark.parametrize("d", [768, 770])
def test_layernorm_large_mean(d):
    """Rows 100 + 2 randn (mean^2 / variance = 2500) against fp64, vector (768) and scalar (770) kernels.  Bound: the
    ordinary tolerance or 8 x the error torch's own fp32 CPU layer_norm + autograd makes on the same rows, whichever is
    larger (8: a differently ordered fp32 sum).  A one-pass variance E[x^2] - E[x]^2 loses 2500 x 6e-8 = 1.5e-4 relative
    in the variance and misses this by two orders of magnitude."""
    R = 77
    x = 100 + 2 * rnd(R, d, seed=41)
    gamma, beta, dy = 1 + 0.1 * rnd(d, seed=42), 0.1 * rnd(d, seed=43), rnd(R, d, seed=44)
    y, dx, _, _, xh = ln_ref64(x, gamma, beta, dy)
    dgamma, dbeta = (dy.double() * xh).sum(0), dy.double().sum(0)
    assert_sensitive(dy.double() * xh, 1e-4, dgamma, "dgamma")
    assert_sensitive(dy.double(), 1e-4, dbeta, "dbeta")
    x32, g32, b32 = (t.clone().requires_grad_(True) for t in (x, gamma, beta))
    y32 = torch.nn.functional.layer_norm(x32, (d,), g32, b32, 1e-5)
    (y32 * dy).sum().backward()
    e = {k: 8 * (a.detach().double() - b).abs().max().item()
         for k, a, b in (("y", y32, y), ("dx", x32.grad, dx), ("dgamma", g32.grad, dgamma), ("dbeta", b32.grad, dbeta))}
    xd, gd, bd, dyd = (t.to(DEV) for t in (x, gamma, beta, dy))
    out, outf = ct_out(R, pad32(d), dtype=BPM_F32), Guarded(R, d)
    mean, rstd, mean2, rstd2 = (Guarded(R) for _ in range(4))
    ops.ln_fwd(BPM_F32, [ops.ln_problem(xd, gd, bd, mean.v, rstd.v, R, out=out.v, ldo=pad32(d)),
                         ops.ln_problem(xd, gd, bd, mean2.v, rstd2.v, R, out=outf.v, ldo=d, out_f32=True)], d)
    close_or(out.v[:, :d], y, 2e-5, e["y"], "large mean y (CT f32)")
    close_or(outf.v, y, 2e-5, e["y"], "large mean y")
    dxo, dgam, dbet = Guarded(R, d), Guarded(d, start=torch.zeros(d)), Guarded(d, start=torch.zeros(d))
    ops.ln_bwd([ops.ln_problem(xd, gd, None, mean.v, rstd.v, R, dy=dyd, ldy=d, dx=dxo.v, dgamma=dgam.v, dbeta=dbet.v)], d)
    close_or(dxo.v, dx, 1e-4, e["dx"], "large mean dx")
    close_or(dgam.v, dgamma, 1e-4, e["dgamma"], "large mean dgamma")
    close_or(dbet.v, dbeta, 1e-4, e["dbeta"], "large mean dbeta")
    for g in (out, outf, mean, rstd, mean2, rstd2, dxo, dgam, dbet):
        g.check("large mean")


# ---------------------------------------------------------------------------
# 2. The workspace hand-off of bpm_ln_bwd_ws
# ---------------------------------------------------------------------------
HO_R = (1037, 1, 2, 520, 9, 64)      # tickets are per problem: the small ones finish while the large ones run
HO_D = 768
HO_SEED = 77


@functools.lru_cache(maxsize=1)
def handoff_case():
    d, probs = HO_D, []
    for i, R in enumerate(HO_R):
        p = SimpleNamespace(R=R, site=9 + i)
        p.x = rnd(R, d, seed=410 + i) * 2 + 0.5
        p.dy = rnd(R, d, seed=440 + i)
        p.gamma = 1 + 0.1 * rnd(d, seed=420 + i)
        _, p.dx, mu, rs, xh = ln_ref64(p.x, p.gamma, None, p.dy)
        p.mean, p.rstd = mu.float(), rs.float()
        p.g0, p.b0, p.c0 = rnd(d, seed=460 + i), rnd(d, seed=470 + i), rnd(d, seed=480 + i)
        p.cg, p.cb = p.dy.double() * xh, p.dy.double()
        p.mult = drop_mult((R, d), LN_P, HO_SEED, p.site)
        p.cast = p.dx * p.mult.double()
        p.dgamma, p.dbeta, p.csum = p.g0.double() + p.cg.sum(0), p.b0.double() + p.cb.sum(0), p.c0.double() + p.cast.sum(0)
        assert_sensitive(p.cg, 1e-4, p.dgamma, f"dgamma {i}")
        assert_sensitive(p.cb, 1e-4, p.dbeta, f"dbeta {i}")
        assert_sensitive(p.cast, 1e-4, p.csum, f"cast_colsum {i}")
        probs.append(p)
    return probs


class HandoffLaunch:
    """The six problems on the device; outputs are Guarded so that a launch can be repeated from the same start."""

    def __init__(self, grads=None, csums=None, skew=0):
        d = HO_D
        self.ref = handoff_case()
        n = len(self.ref)
        self.grads = [True] * n if grads is None else grads
        self.csums = [True] * n if csums is None else csums
        self.keep = [[t.to(DEV) for t in (p.x, p.gamma, p.mean, p.rstd, p.dy)] for p in self.ref]
        self.dx = [Guarded(p.R, d) for p in self.ref]
        self.cast = [ct_out(p.R, d, dtype=BPM_BF16) for p in self.ref]
        self.dgam = [Guarded(d, start=p.g0, skew=skew) for p in self.ref]
        self.dbet = [Guarded(d, start=p.b0, skew=skew) for p in self.ref]
        self.cs = [Guarded(d, start=p.c0) for p in self.ref]
        self.share = {}
        self.ws = torch.zeros((_lib.lib().bpm_ln_bwd_ws_bytes(n, d) + 3) // 4, device=DEV)

    def outputs(self):
        return self.dx + self.cast + self.dgam + self.dbet + self.cs

    def problems(self):
        out = []
        for i, (p, (x, gamma, mean, rstd, dy)) in enumerate(zip(self.ref, self.keep)):
            j = self.share.get(i, i)                 # problem i adds into problem j's dgamma / dbeta
            out.append(ops.ln_problem(x, gamma, None, mean, rstd, p.R, dy=dy, ldy=HO_D, dx=self.dx[i].v,
                                      dgamma=self.dgam[j].v if self.grads[i] else None, dbeta=self.dbet[j].v if self.grads[i] else None,
                                      cast=self.cast[i].v, ldc=HO_D, cast_colsum=self.cs[i].v if self.csums[i] else None,
                                      drop_p=LN_P, drop_site=p.site))
        return out

    def run(self, ws=True):
        arr = ops.array(_lib.LnProblem, self.problems())
        L, s = _lib.lib(), torch.cuda.current_stream().cuda_stream
        if ws:
            _lib.check(L.bpm_ln_bwd_ws(BPM_BF16, arr, len(arr), HO_D, HO_SEED, self.ws.data_ptr(), self.ws.numel() * 4, s), "bpm_ln_bwd_ws")
        else:
            _lib.check(L.bpm_ln_bwd(BPM_BF16, arr, len(arr), HO_D, HO_SEED, s), "bpm_ln_bwd")
        torch.cuda.synchronize()
        # the ticket words in front of the partial rows are zero again after every launch
        assert not self.ws[:64].view(torch.int32).any(), "ticket words left set"
        return [g.v.clone() for g in self.outputs()]

    def check_rows(self):
        for i, p in enumerate(self.ref):
            close(self.dx[i].v, p.dx, 1e-4, f"dx {i}")
            close(self.cast[i].v.float(), p.cast, 1e-2, f"cast {i}")
        for g in self.outputs():
            g.check("ln_bwd_ws")


def test_ln_bwd_ws_six_problems_repeat_bitwise():
    h = HandoffLaunch()
    first = h.run()
    h.check_rows()
    for i, p in enumerate(h.ref):
        close(h.dgam[i].v, p.dgamma, 1e-4, f"dgamma {i}")
        close(h.dbet[i].v, p.dbeta, 1e-4, f"dbeta {i}")
        close(h.cs[i].v, p.csum, 1e-4, f"cast_colsum {i}")
    for rep in range(3):                            # same workspace, outputs reset to the same start
        for g in h.outputs():
            g.reset()
        again = h.run()
        for a, b in zip(first, again):
            assert torch.equal(bits(a), bits(b)), f"repeat {rep + 1} differs"
    # the plain-atomics form: same dx / cast bit for bit, sums within tolerance
    for g in h.outputs():
        g.reset()
    n = len(h.ref)
    raw = h.run(ws=False)
    for a, b in zip(first[:2 * n], raw[:2 * n]):
        assert torch.equal(bits(a), bits(b)), "bpm_ln_bwd: dx / cast differ from the workspace path"
    for i, p in enumerate(h.ref):
        close(h.dgam[i].v, p.dgamma, 1e-4, f"atomics dgamma {i}")
        close(h.dbet[i].v, p.dbeta, 1e-4, f"atomics dbeta {i}")
        close(h.cs[i].v, p.csum, 1e-4, f"atomics cast_colsum {i}")
    for g in h.outputs():
        g.check("bpm_ln_bwd")


def test_ln_bwd_ws_shared_and_unaligned_rows_fall_back_to_atomics():
    # problems 0 and 3 add into the same dgamma / dbeta: detected, atomics, the sum of both
    h = HandoffLaunch()
    h.share = {3: 0}
    h.run()
    h.check_rows()
    a, b = h.ref[0], h.ref[3]
    both_g, both_b = a.dgamma + b.cg.sum(0), a.dbeta + b.cb.sum(0)
    assert_sensitive(torch.cat([a.cg, b.cg]), 1e-4, both_g, "shared dgamma")
    assert_sensitive(torch.cat([a.cb, b.cb]), 1e-4, both_b, "shared dbeta")
    close(h.dgam[0].v, both_g, 1e-4, "shared dgamma")
    close(h.dbet[0].v, both_b, 1e-4, "shared dbeta")
    assert torch.equal(h.dgam[3].v.cpu(), b.g0) and torch.equal(h.dbet[3].v.cpu(), b.b0)       # not passed: untouched
    for i, p in enumerate(h.ref):
        if i not in (0, 3):
            close(h.dgam[i].v, p.dgamma, 1e-4, f"dgamma {i}")
            close(h.dbet[i].v, p.dbeta, 1e-4, f"dbeta {i}")
        close(h.cs[i].v, p.csum, 1e-4, f"cast_colsum {i}")
    # dgamma / dbeta 4 bytes off 16-byte alignment
    h = HandoffLaunch(skew=1)
    assert h.dgam[0].v.data_ptr() % 16 == 4 and h.cs[0].v.data_ptr() % 16 == 0
    h.run()
    h.check_rows()
    for i, p in enumerate(h.ref):
        close(h.dgam[i].v, p.dgamma, 1e-4, f"unaligned dgamma {i}")
        close(h.dbet[i].v, p.dbeta, 1e-4, f"unaligned dbeta {i}")
        close(h.cs[i].v, p.csum, 1e-4, f"unaligned cast_colsum {i}")


def test_ln_bwd_ws_absent_sums():
    """Problem 0 has only cast_colsum, problem 3 no sums at all (its blocks draw no ticket), the others everything."""
    n = len(HO_R)
    grads, csums = [True] * n, [True] * n
    grads[0] = grads[3] = csums[3] = False
    h = HandoffLaunch(grads, csums)
    first = h.run()
    h.check_rows()
    for i, p in enumerate(h.ref):
        if grads[i]:
            close(h.dgam[i].v, p.dgamma, 1e-4, f"dgamma {i}")
            close(h.dbet[i].v, p.dbeta, 1e-4, f"dbeta {i}")
        else:
            assert torch.equal(h.dgam[i].v.cpu(), p.g0) and torch.equal(h.dbet[i].v.cpu(), p.b0)
        if csums[i]:
            close(h.cs[i].v, p.csum, 1e-4, f"cast_colsum {i}")
        else:
            assert torch.equal(h.cs[i].v.cpu(), p.c0)
    for g in h.outputs():
        g.reset()
    for a, b in zip(first, h.run()):
        assert torch.equal(bits(a), bits(b))


# ---------------------------------------------------------------------------
# 3. bpm_rows_cast: column-sum kernel, interleaved CT output
# ---------------------------------------------------------------------------
CS_SHAPES = [(70, 96), (300, 300), (768, 768), (1024, 1024)]        # (C, lda); 1024 columns = 256 chunks, the kernel's limit


@functools.lru_cache(maxsize=None)
def colsum_input(R, C_, kind):
    a = rnd(R, C_, seed=500 + C_ + R)
    ar = a.to(torch.bfloat16).float() if kind == "ct_bf16" else a
    start = rnd(C_, seed=600 + C_)
    ref = start.double() + ar.double().sum(0)
    assert_sensitive(ar, 1e-4, ref, f"colsum R={R} C={C_}")
    return a, start, ref


@pytest.mark.parametrize("swap", [0, 1])
@pytest.mark.parametrize("kind", ["f32", "ct_f32", "ct_bf16"])
def test_rows_cast_column_sums_over_many_row_blocks(kind, swap):
    """Column sums only (colsum_kernel): 129 and 1037 rows (2 and 9 blocks of 128 rows with a ragged last one), four
    problems of different shape in one launch, fp32 and CT inputs, colsum starting non-zero."""
    dtype = BPM_BF16 if kind != "ct_f32" else BPM_F32
    probs, keep, checks = [], [], []
    for k, (C_, lda) in enumerate(CS_SHAPES):
        R = (129, 1037)[(k + swap) % 2]
        a, start, ref = colsum_input(R, C_, kind)
        if kind == "f32":
            ad = torch.zeros(R, lda)
            ad[:, :C_] = a
            ad = ad.to(DEV)
        else:
            lda = max(lda, pad32(C_))
            ad, _ = to_ct(a, dtype, lda)
        cs = Guarded(C_, start=start)
        keep.append(ad)
        probs.append(ops.cast_problem(ad, lda, R, C_, a_is_ct=kind != "f32", colsum=cs.v))
        checks.append((cs, ref, f"colsum {kind} R={R} C={C_}"))
    ops.rows_cast(dtype, probs)
    for cs, ref, what in checks:
        close(cs.v, ref, 1e-4, what)
        cs.check(what)


def test_rows_cast_column_sums_past_the_chunk_limit():
    """C = 1028 is 257 four-column chunks: past colsum_kernel's 256, the general kernel takes it."""
    R, C_ = 129, 1028
    a, start, ref = colsum_input(R, C_, "f32")
    ad, cs = a.to(DEV), Guarded(C_, start=start)
    ops.rows_cast(BPM_F32, [ops.cast_problem(ad, C_, R, C_, colsum=cs.v)])
    close(cs.v, ref, 1e-4, "colsum C=1028")
    cs.check("colsum C=1028")


@pytest.mark.parametrize("dtype", DT)
def test_rows_cast_interleaved_ct_output(dtype):
    """ct_cols: two [R, ld] CT matrices interleaved in one [R, 2 ld] buffer (ldd = 2 ld); a problem writes its own ld
    columns of every row ([C, ld) zeroed) and nothing of its neighbour's."""
    R, C_, ld = 77, 300, 320
    ctt, esz = ops.ct_torch(dtype), 2 if dtype == BPM_BF16 else 4
    tc = 1e-6 if dtype == BPM_F32 else 1e-2
    a = [rnd(R, C_, seed=51 + i) for i in range(2)]
    b = [rnd(R, C_, seed=53 + i) for i in range(2)]
    ad, bd = [t.to(DEV) for t in a], [t.to(DEV) for t in b]
    dst = ct_out(R, 2 * ld, dtype=dtype)
    ops.rows_cast(dtype, [ops.cast_problem(ad[0], C_, R, C_, dst_ct=dst.v, ldd=2 * ld, ct_cols=ld)])
    close(dst.v[:, :C_].float(), a[0].to(ctt).float(), tc, "left half")
    assert (dst.v[:, C_:ld].float() == 0).all()
    assert (dst.v[:, ld:].float() == CT_FILL).all(), "right half written"
    dst.check("ct_cols, left half")

    dst.reset()
    df = [Guarded(R, C_) for _ in range(2)]
    start = [rnd(C_, seed=55 + i) for i in range(2)]
    cs = [Guarded(C_, start=s) for s in start]
    seed, p = 3, 0.1
    ops.rows_cast(dtype, [ops.cast_problem(ad[i], C_, R, C_, b=bd[i], ldb=C_, dst_ct=dst.v.data_ptr() + i * ld * esz, ldd=2 * ld, ct_cols=ld,
                                           dst_f32=df[i].v, ldf=C_, colsum=cs[i].v, drop_p=p, drop_site=9 + i) for i in range(2)], seed=seed)
    for i in range(2):
        ref = (a[i].double() + b[i].double()) * drop_mult((R, C_), p, seed, 9 + i).double()
        csr = start[i].double() + ref.sum(0)
        assert_sensitive(ref, 1e-4, csr, f"colsum half {i}")
        close(df[i].v, ref, 1e-6, f"f32 half {i}")
        close(dst.v[:, i * ld:i * ld + C_].float(), ref.float().to(ctt).float(), tc, f"ct half {i}")
        assert (dst.v[:, i * ld + C_:(i + 1) * ld].float() == 0).all()
        close(cs[i].v, csr, 1e-4, f"colsum half {i}")
        df[i].check("dst_f32")
        cs[i].check("colsum")
    dst.check("ct_cols, both halves")


# ---------------------------------------------------------------------------
# 4. Entry points with no kernel test
# ---------------------------------------------------------------------------
BIG = 2_097_159       # 524 289 quads: past 513 blocks x 1024, so the block loop iterates; 3 trailing elements
ADDN = [(1, 1, None), (1, 8, "first"), (3, 2, "last"), (3, 5, None), (4, 1, "first"), (4, 2, None), (4, 8, "last"), (5, 5, "first"),
        (5, 2, None), (5, 8, None), (4099, 1, None), (4099, 2, "first"), (4099, 5, "last"), (4099, 8, None),
        (BIG, 2, "last"), (BIG, 5, "first"), (BIG, 1, None), (BIG, 8, None)]


def test_add_n():
    """18 problems in one launch: counts with 0-3 trailing elements and one whose block loop iterates, 1 to 8 inputs, out
    aliasing the first or the last input.  The kernel adds in input order: bitwise equal to the fp32 sum in that order."""
    assert len(ADDN) == _lib.MAX_GROUP
    base = [rnd(BIG + 1000, seed=700 + j) for j in range(8)]
    probs, checks = [], []
    for k, (count, n_in, alias) in enumerate(ADDN):
        o = (37 * k) % 1000                                    # different data per problem
        ins = [base[(j + k) % 8][o:o + count].clone() for j in range(n_in)]
        ref = ins[0].clone()
        for t in ins[1:]:
            ref += t
        out = Guarded(count) if alias is None else Guarded(count, start=ins[0 if alias == "first" else -1])
        ind = [t.to(DEV) for t in ins]
        if alias is not None:
            ind[0 if alias == "first" else -1] = out.v
        probs.append(ops.addn_problem(out.v, ind))
        checks.append((out, ref, ins, ind, alias))
    ops.add_n(probs)
    for k, (out, ref, ins, ind, alias) in enumerate(checks):
        assert torch.equal(out.v.cpu(), ref), f"add_n problem {k} {ADDN[k]}"
        out.check(f"add_n problem {k}")
        for j, (t, td) in enumerate(zip(ins, ind)):
            if td is not out.v:
                assert torch.equal(td.cpu(), t), f"add_n problem {k}: input {j} changed"


def test_groups_past_the_launch_limit_reach_the_second_chunk():
    """MAX_GROUP + 1 problems: the wrappers launch MAX_GROUP and then one, and the last problem is read at its own offset
    in the array.  Sums of two small integers and copies are exact: compared bitwise."""
    n = _lib.MAX_GROUP + 1
    a = torch.arange(n * 16, dtype=torch.float32, device=DEV).view(n, 16)
    b = (torch.arange(n * 16, dtype=torch.float32, device=DEV) % 7).view(n, 16) + 1
    out = torch.full((n, 16), -1.0, device=DEV)
    ops.add_n([ops.addn_problem(out[k], [a[k], b[k]]) for k in range(n)])
    assert torch.equal(out, a + b)
    src = torch.arange(n * 2 * 8, dtype=torch.float32, device=DEV).view(n, 2, 8) + 3
    dst = torch.full((n, 2, 8), -1.0, device=DEV)
    ops.rows_cast(BPM_F32, [ops.cast_problem(src[k], 8, 2, 8, dst_f32=dst[k], ldf=8) for k in range(n)])
    assert torch.equal(dst, src)


def test_zero_segments():
    """One table of five segments (1, 2 and 3 blocks of 4096 elements; one segment 4 bytes off 16-byte alignment) in a
    buffer of ones: the segments come back exactly zero, every gap still one."""
    segs = [(64, 1), (128, 3), (256, 4096), (4416, 4097), (8577, 10007)]        # (offset, length) in floats
    buf = torch.ones(8577 + 10007 + 64, device=DEV)
    assert buf.data_ptr() % 16 == 0 and (segs[4][0] * 4) % 16 == 4
    tab, nd, nblk = ops.zero_table([(buf.data_ptr() + 4 * o, n) for o, n in segs])
    assert nblk == 1 + 1 + 1 + 2 + 3
    ops.zero_segments(tab, nd, nblk)
    want = torch.ones(buf.numel())
    for o, n in segs:
        want[o:o + n] = 0.0
    assert torch.equal(buf.cpu(), want)


def split_input(R, C_, seed):
    """randn with +-0, exact ties between two bf16 values (both parities of the kept bit, both signs), values whose low
    part is itself a tie, and a column of large magnitudes."""
    x = rnd(R, C_, seed=seed)
    x[0, :8] = torch.tensor([0.0, -0.0, 1 + 2.0 ** -8, 1 + 3 * 2.0 ** -8, -(1 + 2.0 ** -8), -(1 + 3 * 2.0 ** -8),
                             1 + 2.0 ** -7 + 2.0 ** -16, 3.0e38])
    x[1:, 3] = (1 + 2.0 ** -8) * 2.0 ** torch.arange(1, R).clamp(max=60).float()           # ties at every exponent
    x[1:, 4] = x[1:, 3] * (1 + 2.0 ** -7) * -1.0
    x[2, 5:7] = torch.tensor([2.0 ** -100, -2.0 ** -100 * (1 + 2.0 ** -8)])
    return x


def test_split_rows():
    """hi = bf16(x) and lo = bf16(x - hi) are exact IEEE operations (round to nearest even; the difference is exact):
    bitwise against the same two roundings in torch.  Scalar loads (ld = 35), vector loads, and a column view of a
    three-wide buffer, in one launch."""
    shapes = [(37, 35, 35, 128), (200, 300, 300, 384), (64, 768, 2304, 768)]
    probs, keep, checks = [], [], []
    for k, (R, C_, ld, ldp) in enumerate(shapes):
        x = split_input(R, C_, 800 + k)
        wide = rnd(R, ld, seed=810 + k)
        c0 = 768 if ld > C_ else 0
        wide[:, c0:c0 + C_] = x
        wd = wide.to(DEV)
        dst = Guarded(R, 2 * ldp, dtype=torch.bfloat16, fill=CT_FILL)
        p = _lib.SplitProblem()
        p.src, p.dst, p.R, p.C, p.ld, p.ldp = wd.data_ptr() + 4 * c0, dst.v.data_ptr(), R, C_, ld, ldp
        hi = x.to(torch.bfloat16)
        lo = (x - hi.float()).to(torch.bfloat16)
        assert torch.isfinite(hi.float()).all() and (lo.float() != 0).any()
        want = torch.zeros(R, 2 * ldp, dtype=torch.bfloat16)
        want[:, :C_], want[:, ldp:ldp + C_] = hi, lo
        probs.append(p)
        keep.append(wd)
        checks.append((dst, want, (R, C_, ld, ldp)))
    _lib.check(_lib.lib().bpm_split_rows(ops.array(_lib.SplitProblem, probs), len(probs), torch.cuda.current_stream().cuda_stream), "bpm_split_rows")
    for dst, want, shape in checks:
        got = dst.v.cpu()
        ldp, C_ = shape[3], shape[1]
        assert torch.equal(bits(got[:, :C_]), bits(want[:, :C_])), f"hi {shape}"
        assert torch.equal(bits(got[:, ldp:ldp + C_]), bits(want[:, ldp:ldp + C_])), f"lo {shape}"
        assert torch.equal(bits(got), bits(want)), f"pad columns {shape}"
        dst.check(f"split {shape}")


# three descriptors of different size per table: a plain matrix, a narrow one with an odd row stride, and a 300-row block
# inside a [900, 300] matrix; (rows, cols, row offset inside the parent, parent rows)
TAB = [(600, 300, 0, 600), (96, 35, 0, 96), (300, 300, 300, 900)]


def chained(descs, blocks):
    blk = 0
    for d_, n in zip(descs, blocks):
        d_.blk0 = blk
        blk += n
    return ops.device_table(descs), len(descs), blk


@pytest.mark.parametrize("dtype", DT)
def test_pack_weights_table_of_three(dtype):
    ctt = ops.ct_torch(dtype)
    descs, keep, checks = [], [], []
    for k, (rows, cols, r0, prows) in enumerate(TAB):
        ld = pad32(cols)
        W = rnd(prows, cols, seed=900 + k)
        gamma = (1 + 0.2 * rnd(cols, seed=910 + k)) if k != 1 else None
        Wd, gd = W.to(DEV), gamma.to(DEV) if gamma is not None else None
        shadow = ct_out(prows, ld, dtype=dtype)
        pd = _lib.PackDesc()
        pd.src, pd.dst = Wd.data_ptr() + 4 * r0 * cols, shadow.v.data_ptr() + shadow.v.element_size() * r0 * ld
        pd.rows, pd.cols, pd.ld, pd.src_ld, pd.dst_ld = rows, cols, ld, cols, ld
        pd.colscale = gd.data_ptr() if gd is not None else None
        blk = W[r0:r0 + rows]
        want = torch.full((prows, ld), CT_FILL, dtype=ctt)
        want[r0:r0 + rows] = 0
        want[r0:r0 + rows, :cols] = (blk * gamma if gamma is not None else blk).to(ctt)       # one fp32 multiply, one rounding: exact
        descs.append(pd)
        keep += [Wd, gd]
        checks.append((shadow, want))
    tab, nd, nblk = chained(descs, [(r * pad32(c) + 1023) // 1024 for r, c, _, _ in TAB])
    ops.pack_weights(dtype, tab, nd, nblk)
    for k, (shadow, want) in enumerate(checks):
        assert torch.equal(bits(shadow.v.cpu()), bits(want)), f"pack_weights descriptor {k}"
        shadow.check(f"pack_weights descriptor {k}")


def test_fold_bias_table_of_three():
    descs, keep, checks = [], [], []
    for k, (rows, cols, r0, prows) in enumerate(TAB):
        W = rnd(prows, cols, seed=920 + k) * cols ** -0.5
        beta, b = 0.2 * rnd(cols, seed=930 + k), (0.1 * rnd(rows, seed=940 + k) if k != 1 else None)
        Wd, btd, bd = W.to(DEV), beta.to(DEV), b.to(DEV) if b is not None else None
        out = Guarded(rows)
        fd = _lib.FoldDesc()
        fd.W, fd.beta, fd.b, fd.out = Wd.data_ptr() + 4 * r0 * cols, btd.data_ptr(), bd.data_ptr() if bd is not None else None, out.v.data_ptr()
        fd.rows, fd.cols, fd.ldw = rows, cols, cols
        ref = W[r0:r0 + rows].double() @ beta.double() + (b.double() if b is not None else 0.0)
        descs.append(fd)
        keep += [Wd, btd, bd]
        checks.append((out, ref))
    tab, nd, nblk = chained(descs, [(r + 3) // 4 for r, _, _, _ in TAB])
    ops.fold_bias(tab, nd, nblk)
    for k, (out, ref) in enumerate(checks):
        close(out.v, ref, 1e-5, f"folded bias {k}")
        out.check(f"folded bias {k}")


@pytest.mark.parametrize("store_dw", [False, True])
def test_unfold_grads_table_of_three(store_dw):
    """dW (+)= dWf gamma + dbf beta, dbias += dbf, dgamma += sum_n dWf W, dbeta += sum_n dbf W over three descriptors
    (300 rows = 18.75 blocks of 16); store_dw: dW is written into NaN, never read."""
    descs, keep, checks = [], [], []
    for k, (rows, cols, r0, prows) in enumerate(TAB):
        W = rnd(prows, cols, seed=950 + k) * cols ** -0.5
        dWf = rnd(rows, cols, seed=960 + k)
        dbf = rnd(rows, seed=970 + k)
        dbf = torch.where(dbf < 0, dbf - 1, dbf + 1)                # |dbf| >= 1: every row counts in dbeta
        gamma, beta = 1 + 0.2 * rnd(cols, seed=980 + k), 0.2 * rnd(cols, seed=990 + k)
        s = [rnd(*sh, seed=1000 + 10 * k + j) for j, sh in enumerate(((prows, cols), (rows,), (cols,), (cols,)))]
        Wd, dWfd, dbfd, gd, btd = (t.to(DEV) for t in (W, dWf, dbf, gamma, beta))
        dW = Guarded(prows, cols) if store_dw else Guarded(prows, cols, start=s[0])
        db, dg, dbt = Guarded(rows, start=s[1]), Guarded(cols, start=s[2]), Guarded(cols, start=s[3])
        ud = _lib.UnfoldDesc()
        ud.dWf, ud.dbf, ud.W, ud.gamma, ud.beta = dWfd.data_ptr(), dbfd.data_ptr(), Wd.data_ptr() + 4 * r0 * cols, gd.data_ptr(), btd.data_ptr()
        ud.dW, ud.dbias, ud.dgamma, ud.dbeta = dW.v.data_ptr() + 4 * r0 * cols, db.v.data_ptr(), dg.v.data_ptr(), dbt.v.data_ptr()
        ud.rows, ud.cols, ud.ldw = rows, cols, cols
        Wb = W[r0:r0 + rows].double()
        r = SimpleNamespace(r0=r0, rows=rows, start=s[0])
        r.dW = dWf.double() * gamma.double() + dbf.double()[:, None] * beta.double()
        if not store_dw:
            r.dW = r.dW + s[0][r0:r0 + rows].double()
        cg, cb = dWf.double() * Wb, dbf.double()[:, None] * Wb
        r.db, r.dg, r.dbt = s[1].double() + dbf.double(), s[2].double() + cg.sum(0), s[3].double() + cb.sum(0)
        assert_sensitive(cg, 2e-4, r.dg, f"unfold dgamma {k}")
        assert_sensitive(cb, 2e-4, r.dbt, f"unfold dbeta {k}")
        descs.append(ud)
        keep += [Wd, dWfd, dbfd, gd, btd]
        checks.append((dW, db, dg, dbt, r))
    tab, nd, nblk = chained(descs, [(r + 15) // 16 for r, _, _, _ in TAB])
    ops.unfold_grads(tab, nd, nblk, store_dw=store_dw)
    for k, (dW, db, dg, dbt, r) in enumerate(checks):
        got = dW.v.cpu()
        blk = got[r.r0:r.r0 + r.rows]
        assert torch.isfinite(blk).all(), f"unfolded dW {k}: not written"
        close(blk, r.dW, 2e-4, f"unfolded dW {k}")
        rest = torch.ones(got.shape[0], dtype=torch.bool)
        rest[r.r0:r.r0 + r.rows] = False
        if store_dw:
            assert torch.isnan(got[rest]).all(), f"unfolded dW {k}: rows outside the block written"
        else:
            assert torch.equal(got[rest], r.start[rest]), f"unfolded dW {k}: rows outside the block changed"
        close(db.v, r.db, 2e-4, f"unfolded dbias {k}")
        close(dg.v, r.dg, 2e-4, f"unfolded dgamma {k}")
        close(dbt.v, r.dbt, 2e-4, f"unfolded dbeta {k}")
        for g in (dW, db, dg, dbt):
            g.check(f"unfold_grads descriptor {k}")


def embed_ref(x, table, scale, pos0, stride, mult):
    T = x.shape[0]
    pos = torch.where(x[:, :, 0] != 0, pos0 + stride * torch.arange(T)[:, None] + 1, torch.zeros(1, dtype=torch.long))
    return (scale * x.double() + table.double()[pos]) * mult.double()


def test_embed_pos_elementwise_path():
    """d = 50 (d % 4 != 0) takes the element-wise loops: forward with dropout and pos_stride 2, backward with and
    without accumulation.  At d = 24, x / out views 4 bytes off alignment take them too and must reproduce the vector
    path's result bit for bit."""
    from oracle import bpmult_cpu as O
    T, B, d, p, seed, stride = 9, 3, 50, 0.25, 1, 2
    scale = math.sqrt(d)
    x = rnd(T, B, d, seed=33)
    x[2, 1, 0] = 0.0
    x[-2:] = 0.0
    table = O.sinusoid_table(stride * (T - 1) + 2, d)
    mult = drop_mult((T, B, d), p, seed, 4)
    xd, td, out = x.to(DEV), table.to(DEV), Guarded(T, B, d)
    ops.embed_pos_fwd([ops.embed_problem(xd, out.v, T, B, drop_p=p, drop_site=4, pos_stride=stride)], td, d, scale, seed=seed)
    close(out.v, embed_ref(x, table, scale, 0, stride, mult), 1e-6, "embed_pos fwd d=50")
    out.check("embed_pos fwd")
    dy = rnd(T, B, d, seed=34)
    dyd = dy.to(DEV)
    dxa, dxs = Guarded(T, B, d, start=torch.ones(T, B, d)), Guarded(T, B, d)
    ops.embed_pos_bwd([ops.embed_problem(dyd, dxa.v, T, B, accumulate=True, drop_p=p, drop_site=4, pos_stride=stride),
                       ops.embed_problem(dyd, dxs.v, T, B, drop_p=p, drop_site=4, pos_stride=stride)], d, scale, seed=seed)
    close(dxa.v, 1.0 + scale * dy.double() * mult.double(), 1e-6, "embed_pos bwd d=50, accumulate")
    close(dxs.v, scale * dy.double() * mult.double(), 1e-6, "embed_pos bwd d=50")
    dxa.check("embed_pos bwd")
    dxs.check("embed_pos bwd")

    d = 24
    scale = math.sqrt(d)
    x = rnd(T, B, d, seed=35)
    x[3, 0, 0] = 0.0
    table = O.sinusoid_table(stride * (T - 1) + 2, d)
    td = table.to(DEV)
    res = []
    for skew in (0, 1):
        xin, out, dx = Guarded(T, B, d, start=x, skew=skew), Guarded(T, B, d, skew=skew), Guarded(T, B, d, start=torch.ones(T, B, d), skew=skew)
        assert xin.v.data_ptr() % 16 == 4 * skew and out.v.data_ptr() % 16 == 4 * skew
        ops.embed_pos_fwd([ops.embed_problem(xin.v, out.v, T, B, drop_p=p, drop_site=4, pos_stride=stride)], td, d, scale, seed=seed)
        ops.embed_pos_bwd([ops.embed_problem(xin.v, dx.v, T, B, accumulate=True, drop_p=p, drop_site=4)], d, scale, seed=seed)
        out.check("embed_pos fwd d=24")
        dx.check("embed_pos bwd d=24")
        res.append((out.v.clone(), dx.v.clone()))
    close(res[0][0], embed_ref(x, table, scale, 0, stride, drop_mult((T, B, d), p, seed, 4)), 1e-6, "embed_pos fwd d=24")
    assert torch.equal(bits(res[0][0]), bits(res[1][0])), "embed_pos fwd: element-wise path differs from the vector path"
    assert torch.equal(bits(res[0][1]), bits(res[1][1])), "embed_pos bwd: element-wise path differs from the vector path"


@pytest.mark.parametrize("dtype", DT)
def test_pack_rows_past_the_block_cap(dtype):
    """8 x 700 x 384 padded elements = 2100 blocks of 1024: past the 2048-block cap, the loops iterate."""
    B, T, Cn, ld, p, seed = 8, 700, 375, 384, 0.25, 5
    ctt = ops.ct_torch(dtype)
    src = rnd(B, T, Cn, seed=31)
    mult = drop_mult((B, T, Cn), p, seed, 2)
    srcd, dst = src.to(DEV), ct_out(T * B, ld, dtype=dtype)
    ops.pack_rows_fwd(dtype, [ops.pack_problem(B, T, Cn, ld, src=srcd, dst=dst.v, drop_p=p, drop_site=2)], seed=seed)
    ref = (src * mult).permute(1, 0, 2).reshape(T * B, Cn)
    close(dst.v[:, :Cn].float(), ref.to(ctt).float(), 1e-6, "pack fwd")
    assert (dst.v[:, Cn:].float() == 0).all()
    dst.check("pack fwd")
    if dtype == BPM_BF16:
        return                                   # the backward has no CT operand
    g = rnd(T * B, ld, seed=32)
    gd, dsrc = g.to(DEV), Guarded(B, T, Cn)
    ops.pack_rows_bwd([ops.pack_problem(B, T, Cn, 0, g=gd, ldg=ld, dsrc=dsrc.v, drop_p=p, drop_site=2)], seed=seed)
    close(dsrc.v, g[:, :Cn].reshape(T, B, Cn).permute(1, 0, 2) * mult, 1e-6, "pack bwd")
    dsrc.check("pack bwd")


@functools.lru_cache(maxsize=2)
def gmu_case(R, d):
    ts = [rnd(R, d, seed=60 + i).double() for i in range(5)]
    ext = torch.tensor([30.0, -30.0, 100.0, -100.0], dtype=torch.float64)
    for k in range(3):                                   # +-30 and +-100 in a1, a2, ag: alone, and all three together
        ts[k][k, :4] = ext
        ts[k][3, 4 * k:4 * k + 4] = ext
        ts[k][4, :4] = ext.roll(k)
    ts = [t.float().double().requires_grad_(True) for t in ts]
    a1, a2, ag, x1, x2 = ts
    z = torch.sigmoid(ag)
    y = z * torch.tanh(a1) * x1 + (1 - z) * torch.tanh(a2) * x2
    dout = rnd(R, d, seed=66)
    (y * dout.double()).sum().backward()
    return [t.detach().float() for t in ts], y.detach(), dout, [t.grad for t in ts]


@pytest.mark.parametrize("dtype", DT)
@pytest.mark.parametrize("R,d,ldg", [(2750, 768, 768), (77, 25, 32)])
def test_gmu_past_the_block_cap_and_saturated_gates(dtype, R, d, ldg):
    """2750 x 768 = 2 112 000 elements: past 2048 blocks x 1024; d = 25 with ldg = 32: pad columns.  Gate inputs of
    +-30 and +-100 saturate tanh and the sigmoid: finite, and equal to fp64."""
    ins, y, dout, grads = gmu_case(R, d)
    dv = [t.to(DEV) for t in ins]
    out = Guarded(R, d)
    ops.gmu2_fwd([ops.gmu_problem(*dv, R, out=out.v)], d)
    close(out.v, y, 1e-5, "gmu fwd")
    out.check("gmu fwd")
    das = [ct_out(R, ldg, dtype=dtype) for _ in range(3)]
    dx1, dx2 = Guarded(R, d), Guarded(R, d)
    doutd = dout.to(DEV)
    ops.gmu2_bwd(dtype, [ops.gmu_problem(*dv, R, dout=doutd, da1=das[0].v, da2=das[1].v, dag=das[2].v, ldg=ldg, dx1=dx1.v, dx2=dx2.v)], d)
    t = 1e-5 if dtype == BPM_F32 else 1e-2
    for got, ref, nm in zip(das, grads[:3], ("da1", "da2", "dag")):
        close(got.v[:, :d].float(), ref, t, nm)
        assert (got.v[:, d:].float() == 0).all()
        got.check(nm)
    close(dx1.v, grads[3], 1e-5, "dx1")
    close(dx2.v, grads[4], 1e-5, "dx2")
    dx1.check("dx1")
    dx2.check("dx2")
