"""The wide path of unfold_grads (csrc/rows_pack.hip: four columns per thread, the rows' 16-byte loads batched) and the
four-channel path of embed_pos past its grid cap.

unfold_grads: one table of four descriptors, so the binary search, the wide path and both reasons for the one-column path
meet in one launch; fp64 references from the formulas at bpm_unfold_desc.  Every output is a view into a sentinel-filled
buffer (NaN when the launch is the first writer), inside a parent matrix with a row above and below the block.
embed_pos: bitwise against the fp32 restatement (one fused multiply-add, then the mask of the numpy dropout hash), past
the 2048-block grid, so that every thread iterates and the last iteration is a partial one.

The element count the wide embed case was specified with, 2 * 2^20 + 4 * 1000 + 4, is no multiple of d = 8; the case
uses the next size up that is, 2^21 + 4 * 1002 (52529 x 5 rows).
"""
import functools
import math
from types import SimpleNamespace

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import _lib, ops  # noqa: E402
from test_kernels_gpu import DEV, close, drop_mult, rnd  # noqa: E402

NAN = float("nan")
G = 64                         # guard elements on either side of a view (256 bytes: keeps the view's alignment)


def bits(t):
    return t.detach().cpu().contiguous().view(torch.int32)


class Guarded:
    """fp32 tensor as a view into a larger sentinel-filled buffer, `skew` floats past a 16-byte boundary."""

    def __init__(self, *shape, fill=NAN, skew=0, start=None):
        self.n = int(np.prod(shape))
        self.lo = G + skew
        self.buf = torch.full((self.lo + self.n + G,), fill, device=DEV)
        assert self.buf.data_ptr() % 16 == 0
        self.v = self.buf[self.lo:self.lo + self.n].view(*shape)
        if start is not None:
            self.v.copy_(start)
        self.init = self.buf.clone()

    def check(self, what):
        got, was = bits(self.buf), bits(self.init)
        assert torch.equal(got[:self.lo], was[:self.lo]), what + ": bytes in front of the tensor were written"
        assert torch.equal(got[self.lo + self.n:], was[self.lo + self.n:]), what + ": bytes behind the tensor were written"


def assert_sensitive(contrib, t, ref, what):
    """contrib: fp64 [rows, cols] contribution of every row to a column sum with reference `ref`, compared at
    t * max(1, |ref|max): every row's largest contribution is ten times that, so one lost or doubled row shows."""
    bound = 10 * t * max(1.0, ref.abs().max().item())
    low = contrib.abs().amax(1).min().item()
    assert low >= bound, f"{what}: smallest single-row contribution {low:.3e} < 10 x tolerance {bound:.3e}"


# ---------------------------------------------------------------------------------------------------------------------
# unfold_grads
# ---------------------------------------------------------------------------------------------------------------------
# (rows, cols, ldw, floats by which dWf / dW sit past a 16-byte boundary)
UNF = {
    "a": (17, 8, 8, 0),            # wide; two blocks, the second with one live row
    "b": (33, 1028, 1032, 0),      # wide; a second column pass (1028 > 4 * 256), ldw != cols, three blocks, a one-row batch
    "c": (16, 6, 6, 0),            # cols % 4 != 0: one column per thread
    "d": (20, 8, 8, 1),            # dWf and dW 4 bytes off: one column per thread
}
TOL = 2e-4


@functools.lru_cache(maxsize=None)
def unf_data(name):
    """Host inputs and fp64 references of one descriptor (never modified)."""
    rows, cols, ldw, _ = UNF[name]
    k = "abcd".index(name)
    r = SimpleNamespace(rows=rows, cols=cols, ldw=ldw, prows=rows + 2)
    r.W = rnd(r.prows, ldw, seed=2000 + k) * cols ** -0.5
    r.dWf = rnd(rows, cols, seed=2010 + k)
    dbf = rnd(rows, seed=2020 + k)
    r.dbf = torch.where(dbf < 0, dbf - 1, dbf + 1)                 # |dbf| >= 1: every row counts in dbeta
    r.gamma, r.beta = 1 + 0.2 * rnd(cols, seed=2030 + k), 0.2 * rnd(cols, seed=2040 + k)
    r.s_dW, r.s_db = rnd(r.prows, ldw, seed=2050 + k), rnd(rows, seed=2060 + k)
    r.s_dg, r.s_dbt = rnd(cols, seed=2070 + k), rnd(cols, seed=2080 + k)
    Wb, f, db = r.W[1:1 + rows, :cols].double(), r.dWf.double(), r.dbf.double()
    r.upd = f * r.gamma.double() + db[:, None] * r.beta.double()    # dW (+)= this
    r.cg, r.cb = f * Wb, db[:, None] * Wb                            # rows of the dgamma / dbeta sums
    return r


class UnfoldRun:
    """Device buffers of one descriptor: the block is rows [1, 1 + rows) of a [rows + 2, ldw] parent."""

    def __init__(self, name, store_dw, skew=None, skew_w=0, zero_sums=False):
        r = self.r = unf_data(name)
        skew = UNF[name][3] if skew is None else skew
        self.store_dw = store_dw
        self.W = Guarded(r.prows, r.ldw, start=r.W, skew=skew_w)
        self.dWf = Guarded(r.rows, r.cols, start=r.dWf, skew=skew)
        self.dW = Guarded(r.prows, r.ldw, skew=skew) if store_dw else Guarded(r.prows, r.ldw, start=r.s_dW, skew=skew)
        self.db = Guarded(r.rows, start=r.s_db)
        z = torch.zeros(r.cols)
        self.dg, self.dbt = Guarded(r.cols, start=z if zero_sums else r.s_dg), Guarded(r.cols, start=z if zero_sums else r.s_dbt)
        self.keep = [t.to(DEV) for t in (r.dbf, r.gamma, r.beta)]
        ud = self.desc = _lib.UnfoldDesc()
        ud.dWf, ud.dbf, ud.W = self.dWf.v.data_ptr(), self.keep[0].data_ptr(), self.W.v.data_ptr() + 4 * r.ldw
        ud.gamma, ud.beta = self.keep[1].data_ptr(), self.keep[2].data_ptr()
        ud.dW, ud.dbias, ud.dgamma, ud.dbeta = self.dW.v.data_ptr() + 4 * r.ldw, self.db.v.data_ptr(), self.dg.v.data_ptr(), self.dbt.v.data_ptr()
        ud.rows, ud.cols, ud.ldw = r.rows, r.cols, r.ldw
        self.wide = (r.cols % 4 == 0 and r.ldw % 4 == 0 and
                     all(p % 16 == 0 for p in (ud.dWf, ud.W, ud.dW, ud.gamma, ud.beta, ud.dgamma, ud.dbeta)))

    def check(self, what):
        r = self.r
        got, was = self.dW.v.cpu(), self.dW.init[self.dW.lo:self.dW.lo + self.dW.n].view(r.prows, r.ldw).cpu()
        blk = got[1:1 + r.rows, :r.cols]
        assert torch.isfinite(blk).all(), f"{what}: dW not written everywhere"
        close(blk, r.upd if self.store_dw else r.upd + r.s_dW[1:1 + r.rows, :r.cols].double(), TOL, f"{what}: dW")
        outside = torch.ones(r.prows, r.ldw, dtype=torch.bool)
        outside[1:1 + r.rows, :r.cols] = False                      # the rows around the block and its ldw - cols pad columns
        assert torch.equal(bits(got)[outside], bits(was)[outside]), f"{what}: dW changed outside the block"
        close(self.db.v, r.s_db.double() + r.dbf.double(), TOL, f"{what}: dbias")
        close(self.dg.v, r.s_dg.double() + r.cg.sum(0), TOL, f"{what}: dgamma")
        close(self.dbt.v, r.s_dbt.double() + r.cb.sum(0), TOL, f"{what}: dbeta")
        for g in (self.dW, self.db, self.dg, self.dbt):
            g.check(what)
        assert torch.equal(bits(self.W.buf), bits(self.W.init)) and torch.equal(bits(self.dWf.buf), bits(self.dWf.init)), f"{what}: an input was written"


def launch_unfold(runs, store_dw):
    blk = 0
    for u in runs:
        u.desc.blk0 = blk
        blk += (u.r.rows + 15) // 16
    tab = ops.device_table([u.desc for u in runs])
    ops.unfold_grads(tab, len(runs), blk, store_dw=store_dw)
    torch.cuda.synchronize()


@pytest.mark.parametrize("store_dw", [False, True])
def test_unfold_grads_wide_and_narrow_descriptors_in_one_table(store_dw):
    runs = [UnfoldRun(n, store_dw) for n in "abcd"]
    assert [u.wide for u in runs] == [True, True, False, False]
    for n, u in zip("abcd", runs):
        r = u.r
        assert_sensitive(r.cg, TOL, r.s_dg.double() + r.cg.sum(0), f"unfold {n} dgamma")
        assert_sensitive(r.cb, TOL, r.s_dbt.double() + r.cb.sum(0), f"unfold {n} dbeta")
    launch_unfold(runs, store_dw)
    for n, u in zip("abcd", runs):
        u.check(f"unfold_grads descriptor {n} store_dw={int(store_dw)}")


@pytest.mark.parametrize("store_dw", [False, True])
def test_unfold_grads_wide_path_equals_the_one_column_path_bitwise(store_dw):
    """Descriptor (a) twice: aligned (four columns per thread) and with dWf, W and dW one float past a 16-byte boundary (one
    column per thread).  Same expressions, same row order: dW and dbias are equal bit for bit, and so are dgamma / dbeta
    when they start from zero (two blocks: the sum of two terms does not depend on their order)."""
    wide, narrow = UnfoldRun("a", store_dw, skew=0, zero_sums=True), UnfoldRun("a", store_dw, skew=1, skew_w=1, zero_sums=True)
    assert wide.wide and not narrow.wide
    launch_unfold([wide], store_dw)
    launch_unfold([narrow], store_dw)
    r = wide.r
    for what, a, b in (("dW", wide.dW, narrow.dW), ("dbias", wide.db, narrow.db), ("dgamma", wide.dg, narrow.dg), ("dbeta", wide.dbt, narrow.dbt)):
        assert torch.equal(bits(a.v), bits(b.v)), f"unfold_grads {what}: the wide path differs from the one-column path"
    close(wide.dW.v[1:1 + r.rows], r.upd if store_dw else r.upd + r.s_dW[1:1 + r.rows].double(), TOL, "unfold_grads wide dW")
    close(wide.dg.v, r.cg.sum(0), TOL, "unfold_grads wide dgamma")
    close(wide.dbt.v, r.cb.sum(0), TOL, "unfold_grads wide dbeta")


# ---------------------------------------------------------------------------------------------------------------------
# embed_pos
# ---------------------------------------------------------------------------------------------------------------------
D = 8
SCALE = math.sqrt(D)
SEED = 5
# (T, B, pos0, pos_stride, dropout site)
BIG = (52529, 5, 0, 1, 4)        # 2^21 + 4008 elements: the 2048-block grid once, then 1002 quads (501 rows) more
SMALL = (3, 2, 1, 2, 9)          # pad rows, rows two time steps apart starting at step 1


@functools.lru_cache(maxsize=None)
def emb_data(case):
    """Host inputs of one problem (never modified): x with pad rows, dy, the dx start, the table."""
    from oracle import bpmult_cpu as O
    T, B, pos0, stride, site = case
    r = SimpleNamespace(T=T, B=B, pos0=pos0, stride=stride, site=site)
    r.x = rnd(T, B, D, seed=3000 + site)
    r.x[1, 0, 0] = 0.0                      # a pad row with live channels behind its first
    r.x[T - 1, B - 1] = 0.0                 # a pad row of zeros, the problem's last row
    r.x[T // 2, :, 0] = 0.0
    r.dy, r.dx0 = rnd(T, B, D, seed=3100 + site), rnd(T, B, D, seed=3200 + site)
    r.table = O.sinusoid_table(pos0 + stride * (T - 1) + 2, D)
    r.pos = torch.where(r.x[:, :, 0] != 0, pos0 + stride * torch.arange(T)[:, None] + 1, torch.zeros(1, dtype=torch.long))
    assert (r.pos == 0).sum() >= B + 1 and r.pos.max() == pos0 + stride * (T - 1) + 1
    return r


def emb_fwd_ref(r, p):
    """fp32 fused multiply-add (the exact sum rounded once; fp64 holds it but for ties nobody meets), then the mask."""
    s = torch.tensor(SCALE, dtype=torch.float32).double()
    v = (s * r.x.double() + r.table.double()[r.pos]).float()
    return v * drop_mult((r.T, r.B, D), p, SEED, r.site)


def emb_bwd_ref(r, p, accumulate):
    v = (torch.tensor(SCALE, dtype=torch.float32) * r.dy) * drop_mult((r.T, r.B, D), p, SEED, r.site)
    return r.dx0 + v if accumulate else v


def run_fwd(cases, p):
    rs = [emb_data(c) for c in cases]
    table = max((r.table for r in rs), key=len).to(DEV)            # (sinusoid rows do not depend on the table's length)
    xs, outs = [r.x.to(DEV) for r in rs], [Guarded(r.T, r.B, D) for r in rs]
    ops.embed_pos_fwd([ops.embed_problem(x, o.v, r.T, r.B, drop_p=p, drop_site=r.site, pos0=r.pos0, pos_stride=r.stride)
                       for r, x, o in zip(rs, xs, outs)], table, D, SCALE, seed=SEED)
    torch.cuda.synchronize()
    for k, (r, o) in enumerate(zip(rs, outs)):
        assert torch.equal(bits(o.v), bits(emb_fwd_ref(r, p))), f"embed_pos fwd problem {k} p={p}"
        o.check(f"embed_pos fwd problem {k}")


def run_bwd(cases, p, accumulate):
    rs = [emb_data(c) for c in cases]
    dys = [r.dy.to(DEV) for r in rs]
    dxs = [Guarded(r.T, r.B, D, start=r.dx0) if accumulate else Guarded(r.T, r.B, D) for r in rs]
    ops.embed_pos_bwd([ops.embed_problem(dy, dx.v, r.T, r.B, accumulate=accumulate, drop_p=p, drop_site=r.site, pos0=r.pos0, pos_stride=r.stride)
                       for r, dy, dx in zip(rs, dys, dxs)], D, SCALE, seed=SEED)
    torch.cuda.synchronize()
    for k, (r, dx) in enumerate(zip(rs, dxs)):
        assert torch.equal(bits(dx.v), bits(emb_bwd_ref(r, p, accumulate))), f"embed_pos bwd problem {k} p={p} accumulate={accumulate}"
        dx.check(f"embed_pos bwd problem {k}")


@pytest.mark.parametrize("p", [0.0, 0.25])
def test_embed_pos_forward_past_the_grid(p):
    run_fwd([BIG, SMALL], p)


@pytest.mark.parametrize("accumulate", [False, True])
@pytest.mark.parametrize("p", [0.0, 0.25])
def test_embed_pos_backward_past_the_grid(p, accumulate):
    run_bwd([BIG, SMALL], p, accumulate)
