"""The row kernels of deterministic mode on the MI355X.

bpm_unfold_grads_ws (csrc/rows_pack.hip): unfold_grads without float atomics -- dgamma / dbeta from per-block partial
rows, added in block order by the block that finishes last.  bpm_ln_bwd_det (rows_norm.hip) and bpm_rows_cast_ws
(rows_elem.hip), further down: their sections say which shapes and why.

Unfold shapes: 33 rows (three blocks of 16, the last with one live row) by 36 columns (wide path), 37 (one column per thread)
and 1028 (wide, a second pass of 1024 columns); two descriptors per launch.  For each: fp64 references at the tolerance
the existing unfold tests use (tests/test_rowops_streaming_gpu.py, 2e-4 of scale), ten launches from identical inputs
bit-equal, a descriptor alone against the same descriptor in a table of three bit-equal, dW and dbias bit-equal to
bpm_unfold_grads, and the wide path bit-equal to the one-column path from a non-zero start."""
import functools
from types import SimpleNamespace

import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import _lib, ops  # noqa: E402
from test_kernels_gpu import DEV, close, rnd  # noqa: E402
from test_rowops_streaming_gpu import Guarded, assert_sensitive, bits  # noqa: E402

ROWS = 33
# (cols, ldw, floats by which dWf / W / dW sit past a 16-byte boundary)
SHAPES = {"w36": (36, 36, 0), "n37": (37, 37, 0), "w1028": (1028, 1032, 0), "n36": (36, 36, 1)}
TOL = 2e-4


@functools.lru_cache(maxsize=None)
def data(cols, ldw):
    """Host inputs and fp64 references of one descriptor shape (never modified; w36 and n36 share them)."""
    r = SimpleNamespace(rows=ROWS, cols=cols, ldw=ldw)
    r.W = rnd(ROWS, ldw, seed=3000 + cols) * cols ** -0.5
    r.dWf = rnd(ROWS, cols, seed=3010 + cols)
    dbf = rnd(ROWS, seed=3020 + cols)
    r.dbf = torch.where(dbf < 0, dbf - 1, dbf + 1)                 # |dbf| >= 1: every row counts in dbeta
    r.gamma, r.beta = 1 + 0.2 * rnd(cols, seed=3030 + cols), 0.2 * rnd(cols, seed=3040 + cols)
    r.s_dW, r.s_db = rnd(ROWS, ldw, seed=3050 + cols), rnd(ROWS, seed=3060 + cols)
    r.s_dg, r.s_dbt = rnd(cols, seed=3070 + cols), rnd(cols, seed=3080 + cols)
    Wb, f, db = r.W[:, :cols].double(), r.dWf.double(), r.dbf.double()
    r.upd = f * r.gamma.double() + db[:, None] * r.beta.double()
    r.cg, r.cb = f * Wb, db[:, None] * Wb
    return r


class Run:
    """Device buffers of one descriptor, every output inside a sentinel-guarded buffer."""

    def __init__(self, name, store_dw=False):
        cols, ldw, skew = SHAPES[name]
        r = self.r = data(cols, ldw)
        self.store_dw = store_dw
        self.W, self.dWf = Guarded(ROWS, ldw, start=r.W, skew=skew), Guarded(ROWS, cols, start=r.dWf, skew=skew)
        self.dW = Guarded(ROWS, ldw, skew=skew) if store_dw else Guarded(ROWS, ldw, start=r.s_dW, skew=skew)
        self.db, self.dg, self.dbt = Guarded(ROWS, start=r.s_db), Guarded(cols, start=r.s_dg), Guarded(cols, start=r.s_dbt)
        self.keep = [t.to(DEV) for t in (r.dbf, r.gamma, r.beta)]
        ud = self.desc = _lib.UnfoldDesc()
        ud.dWf, ud.dbf, ud.W = self.dWf.v.data_ptr(), self.keep[0].data_ptr(), self.W.v.data_ptr()
        ud.gamma, ud.beta = self.keep[1].data_ptr(), self.keep[2].data_ptr()
        ud.dW, ud.dbias, ud.dgamma, ud.dbeta = self.dW.v.data_ptr(), self.db.v.data_ptr(), self.dg.v.data_ptr(), self.dbt.v.data_ptr()
        ud.rows, ud.cols, ud.ldw = ROWS, cols, ldw
        self.wide = cols % 4 == 0 and ldw % 4 == 0 and all(p % 16 == 0 for p in (ud.dWf, ud.W, ud.dW))

    def outputs(self):
        return {"dW": bits(self.dW.buf), "dbias": bits(self.db.buf), "dgamma": bits(self.dg.buf), "dbeta": bits(self.dbt.buf)}

    def check(self, what):
        r = self.r
        blk = self.dW.v.cpu()[:, :r.cols]
        assert torch.isfinite(blk).all(), f"{what}: dW not written everywhere"
        close(blk, r.upd if self.store_dw else r.upd + r.s_dW[:, :r.cols].double(), TOL, f"{what}: dW")
        close(self.db.v, r.s_db.double() + r.dbf.double(), TOL, f"{what}: dbias")
        close(self.dg.v, r.s_dg.double() + r.cg.sum(0), TOL, f"{what}: dgamma")
        close(self.dbt.v, r.s_dbt.double() + r.cb.sum(0), TOL, f"{what}: dbeta")
        for g in (self.dW, self.db, self.dg, self.dbt):
            g.check(what)
        assert torch.equal(bits(self.W.buf), bits(self.W.init)) and torch.equal(bits(self.dWf.buf), bits(self.dWf.init)), f"{what}: an input was written"


def launch(runs, store_dw=False, ws=True):
    blk = 0
    for u in runs:
        u.desc.blk0 = blk
        blk += (ROWS + 15) // 16
    tab = ops.device_table([u.desc for u in runs])
    if ws:
        ops.unfold_grads_ws(tab, len(runs), blk, max(u.r.cols for u in runs), store_dw=store_dw)
    else:
        ops.unfold_grads(tab, len(runs), blk, store_dw=store_dw)
    torch.cuda.synchronize()


PAIRS = [("w36", "n37"), ("w1028", "n36")]


@pytest.mark.parametrize("store_dw", [False, True])
@pytest.mark.parametrize("pair", PAIRS, ids="+".join)
def test_against_fp64_and_the_default_entry(pair, store_dw):
    runs = [Run(n, store_dw) for n in pair]
    assert [u.wide for u in runs] == [n[0] == "w" for n in pair]
    for n, u in zip(pair, runs):
        assert_sensitive(u.r.cg, TOL, u.r.s_dg.double() + u.r.cg.sum(0), f"unfold {n} dgamma")
        assert_sensitive(u.r.cb, TOL, u.r.s_dbt.double() + u.r.cb.sum(0), f"unfold {n} dbeta")
    launch(runs, store_dw)
    for n, u in zip(pair, runs):
        u.check(f"unfold_grads_ws {n} store_dw={int(store_dw)}")
    # what the workspace route leaves alone: dW and dbias, bit for bit those of bpm_unfold_grads
    ref = [Run(n, store_dw) for n in pair]
    launch(ref, store_dw, ws=False)
    for n, u, v in zip(pair, runs, ref):
        for k in ("dW", "dbias"):
            assert torch.equal(u.outputs()[k], v.outputs()[k]), f"unfold_grads_ws {n}: {k} differs from bpm_unfold_grads"


@pytest.mark.parametrize("pair", PAIRS, ids="+".join)
def test_ten_launches_from_identical_inputs_are_bit_equal(pair):
    first = None
    for k in range(10):
        runs = [Run(n) for n in pair]
        launch(runs)
        got = [u.outputs() for u in runs]
        if first is None:
            first = got
        for n, a, b in zip(pair, first, got):
            for key in a:
                assert torch.equal(a[key], b[key]), f"unfold_grads_ws {n}: {key} of launch {k} differs from launch 0"


@pytest.mark.parametrize("name", sorted(SHAPES))
def test_alone_equals_inside_a_table_of_three(name):
    alone = Run(name)
    launch([alone])
    others = [n for n in ("w1028", "n37", "w36") if n != name][:2]
    for pos in range(3):                                   # first, middle and last descriptor of the table
        mine = Run(name)
        table = [Run(n) for n in others]
        table.insert(pos, mine)
        launch(table)
        for key, a in alone.outputs().items():
            assert torch.equal(a, mine.outputs()[key]), f"unfold_grads_ws {name} at position {pos} of three: {key} differs from the launch alone"


@pytest.mark.parametrize("store_dw", [False, True])
def test_wide_path_equals_the_one_column_path_bitwise(store_dw):
    """36 columns aligned (four columns per thread) and one float past a 16-byte boundary (one column per thread), three
    blocks, sums that start from non-zero values: the partial rows and their block-order sum are the same expressions."""
    wide, narrow = Run("w36", store_dw), Run("n36", store_dw)
    assert wide.wide and not narrow.wide
    launch([wide], store_dw)
    launch([narrow], store_dw)
    for what, a, b in (("dW", wide.dW, narrow.dW), ("dbias", wide.db, narrow.db), ("dgamma", wide.dg, narrow.dg), ("dbeta", wide.dbt, narrow.dbt)):
        assert torch.equal(bits(a.v), bits(b.v)), f"unfold_grads_ws {what}: the wide path differs from the one-column path"


def test_a_too_narrow_max_cols_processes_nothing():
    """The kernel's own guard: a descriptor wider than the partial rows is skipped whole, never written past them."""
    u = Run("w36")
    u.desc.blk0 = 0
    tab = ops.device_table([u.desc])
    ops.unfold_grads_ws(tab, 1, 3, 32)
    torch.cuda.synchronize()
    for g in (u.dW, u.db, u.dg, u.dbt):
        assert torch.equal(bits(g.buf), bits(g.init))


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm backward: bpm_ln_bwd_det
# ---------------------------------------------------------------------------------------------------------------------
# d = 50 and d = 1028 at 1037 rows (the scalar family: partial rows + the finishing launch; 1037 rows are 256 blocks with
# a second, partial iteration), d = 64 (the vector kernels' workspace route, the one every model shape takes), and one
# launch whose two problems share dgamma / dbeta.  Tolerance: 1e-4 of scale, what tests/test_rowops_gpu.py holds the
# atomics path to.
from bpmult_amd._lib import BPM_F32  # noqa: E402
from test_rowops_gpu import ln_ref64  # noqa: E402

LN_R, LN_TOL = 1037, 1e-4


@functools.lru_cache(maxsize=None)
def ln_data(d, R=LN_R, k=0):
    r = SimpleNamespace(d=d, R=R)
    r.x, r.gamma = 2 * rnd(R, d, seed=4000 + d + k) + 0.5, 1 + 0.2 * rnd(d, seed=4010 + d + k)
    r.dy, r.add = rnd(R, d, seed=4020 + d + k), rnd(R, d, seed=4030 + d + k)
    r.s_dg, r.s_db, r.s_cs = rnd(d, seed=4040 + d + k), rnd(d, seed=4050 + d + k), rnd(d, seed=4060 + d + k)
    _, dx, mu, rs, xh = ln_ref64(r.x, r.gamma, None, r.dy)
    r.mean, r.rstd = mu.float(), rs.float()
    r.dx = r.add.double() + dx
    r.dgamma, r.dbeta = (r.dy.double() * xh).sum(0), r.dy.double().sum(0)
    return r


class LnRun:
    def __init__(self, d, R=LN_R, k=0, share=None):
        r = self.r = ln_data(d, R, k)
        ld = (d + 31) // 32 * 32
        self.ins = [t.to(DEV) for t in (r.x, r.gamma, r.mean, r.rstd, r.dy, r.add)]
        self.dx, self.cast = Guarded(R, d), Guarded(R, ld)
        self.dg = share.dg if share else Guarded(d, start=r.s_dg)
        self.db = share.db if share else Guarded(d, start=r.s_db)
        self.cs = Guarded(d, start=r.s_cs)
        x, g, m, s, dy, add = self.ins
        self.p = ops.ln_problem(x, g, None, m, s, R, dy=dy, ldy=d, add=add, dx=self.dx.v, dgamma=self.dg.v, dbeta=self.db.v,
                                cast=self.cast.v, ldc=ld, cast_colsum=self.cs.v, drop_p=0.2, drop_site=9)

    def outputs(self):
        return {k: bits(getattr(self, k).buf) for k in ("dx", "cast", "dg", "db", "cs")}

    def check(self, what):
        r = self.r
        close(self.dx.v, r.dx, LN_TOL, what + ": dx")
        close(self.dg.v, r.s_dg.double() + r.dgamma, LN_TOL, what + ": dgamma")
        close(self.db.v, r.s_db.double() + r.dbeta, LN_TOL, what + ": dbeta")
        cast = self.cast.v[:, :r.d].double().cpu()
        assert float((cast == 0).double().mean()) > 0.1, what + ": the dropout mask drops nothing"
        close(self.cs.v, r.s_cs.double() + cast.sum(0), LN_TOL, what + ": cast_colsum")
        for g in (self.dx, self.cast, self.dg, self.db, self.cs):
            g.check(what)


def ln_launch(runs, det=True):
    ops.ln_bwd([u.p for u in runs], runs[0].r.d, BPM_F32, 77, deterministic=det)
    torch.cuda.synchronize()


@pytest.mark.parametrize("d", [50, 1028, 64])
def test_ln_det_against_fp64_the_default_entry_and_itself(d):
    first = None
    for k in range(10):
        u = LnRun(d)
        ln_launch([u])
        if first is None:
            first = u.outputs()
            u.check(f"ln_bwd_det d={d}")
        for key, a in first.items():
            assert torch.equal(a, u.outputs()[key]), f"ln_bwd_det d={d}: {key} of launch {k} differs from launch 0"
    ref = LnRun(d)
    ln_launch([ref], det=False)                           # what the route leaves alone: dx and the cast output
    for key in ("dx", "cast"):
        assert torch.equal(first[key], ref.outputs()[key]), f"ln_bwd_det d={d}: {key} differs from bpm_ln_bwd_ws"
    if d == 64:                                           # the vector workspace route is the default entry's: the sums too
        for key in ("dg", "db", "cs"):
            assert torch.equal(first[key], ref.outputs()[key]), key


@pytest.mark.parametrize("d", [50, 1028, 64])
def test_ln_det_alone_equals_inside_a_group_of_three(d):
    alone = LnRun(d)
    ln_launch([alone])
    for pos in range(3):
        group = [LnRun(d, R=33, k=1), LnRun(d, R=129, k=2)]
        mine = LnRun(d)
        group.insert(pos, mine)
        ln_launch(group)
        for key, a in alone.outputs().items():
            assert torch.equal(a, mine.outputs()[key]), f"ln_bwd_det d={d} at position {pos} of three: {key} differs from the launch alone"
        group[0 if pos else 1].check(f"ln_bwd_det d={d}, a neighbour of position {pos}")


@pytest.mark.parametrize("d", [50, 64])
def test_ln_det_problems_that_share_dgamma(d):
    """Two problems of one launch add into ONE dgamma / dbeta pair: partial rows added in problem order by one owner."""
    first = None
    for k in range(10):
        a = LnRun(d)
        b = LnRun(d, R=33, k=1, share=a)
        ln_launch([a, b])
        out = {**{"a." + n: t for n, t in a.outputs().items()}, **{"b." + n: t for n, t in b.outputs().items()}}
        if first is None:
            first = out
            close(a.dg.v, a.r.s_dg.double() + a.r.dgamma + b.r.dgamma, LN_TOL, "shared dgamma")
            close(a.db.v, a.r.s_db.double() + a.r.dbeta + b.r.dbeta, LN_TOL, "shared dbeta")
            close(a.dx.v, a.r.dx, LN_TOL, "dx a")
            close(b.dx.v, b.r.dx, LN_TOL, "dx b")
        for key in first:
            assert torch.equal(first[key], out[key]), f"shared dgamma d={d}: {key} of launch {k} differs from launch 0"


# ---------------------------------------------------------------------------------------------------------------------
# rows_cast: bpm_rows_cast_ws
# ---------------------------------------------------------------------------------------------------------------------
# R = 33 and 129 (two and five row blocks of rows_cast_kernel, one and two of colsum_kernel), C = 36 (without dst_ct: the
# vectorised colsum_kernel), 37 and 1028 (rows_cast_kernel: five column blocks), with and without dst_ct.
@functools.lru_cache(maxsize=None)
def cast_data(R, Cn):
    r = SimpleNamespace(R=R, C=Cn)
    r.a, r.s_cs = rnd(R, Cn, seed=5000 + R + Cn), rnd(Cn, seed=5010 + R + Cn)
    return r


class CastRun:
    def __init__(self, R, Cn, ct):
        r = self.r = cast_data(R, Cn)
        self.ct = ct
        ld = (Cn + 31) // 32 * 32
        self.a = r.a.to(DEV)
        self.cs = Guarded(Cn, start=r.s_cs)
        self.dst = Guarded(R, ld) if ct else None
        kw = dict(dst_ct=self.dst.v, ldd=ld, drop_p=0.2, drop_site=4) if ct else {}
        self.p = ops.cast_problem(self.a, Cn, R, Cn, colsum=self.cs.v, **kw)

    def outputs(self):
        out = {"colsum": bits(self.cs.buf)}
        if self.ct:
            out["dst_ct"] = bits(self.dst.buf)
        return out

    def check(self, what):
        r = self.r
        src = self.dst.v[:, :r.C].double().cpu() if self.ct else r.a.double()      # with dst_ct: the sums of what was written
        if self.ct:
            assert float((src == 0).double().mean()) > 0.1, what + ": the dropout mask drops nothing"
            self.dst.check(what)
        close(self.cs.v, r.s_cs.double() + src.sum(0), 1e-4, what + ": colsum")
        self.cs.check(what)


def cast_launch(runs, ws=True):
    (ops.rows_cast_ws if ws else ops.rows_cast)(BPM_F32, [u.p for u in runs], 55)
    torch.cuda.synchronize()


CAST_SHAPES = [(R, Cn) for R in (33, 129) for Cn in (36, 37, 1028)]


@pytest.mark.parametrize("ct", [False, True], ids=["sums-only", "dst_ct"])
@pytest.mark.parametrize("R,Cn", CAST_SHAPES)
def test_rows_cast_ws_against_fp64_the_default_entry_and_itself(R, Cn, ct):
    first = None
    for k in range(10):
        u = CastRun(R, Cn, ct)
        cast_launch([u])
        if first is None:
            first = u.outputs()
            u.check(f"rows_cast_ws {R}x{Cn}")
        for key, a in first.items():
            assert torch.equal(a, u.outputs()[key]), f"rows_cast_ws {R}x{Cn}: {key} of launch {k} differs from launch 0"
    if ct:
        ref = CastRun(R, Cn, ct)
        cast_launch([ref], ws=False)
        assert torch.equal(first["dst_ct"], ref.outputs()["dst_ct"]), "dst_ct differs from bpm_rows_cast"


@pytest.mark.parametrize("ct", [False, True], ids=["sums-only", "dst_ct"])
@pytest.mark.parametrize("R,Cn", CAST_SHAPES)
def test_rows_cast_ws_alone_equals_inside_a_group_of_three(R, Cn, ct):
    alone = CastRun(R, Cn, ct)
    cast_launch([alone])
    # the entry picks ONE kernel per launch, as bpm_rows_cast does (sums only, every problem aligned: colsum_kernel): the
    # neighbours are problems that leave the launch with the kernel the problem takes alone
    if not ct and Cn == 36:
        others = [(162 - R, 36), (162 - R, 36)]
    else:
        others = [s for s in CAST_SHAPES if s != (R, Cn) and (ct or s[1] != 36)]
        others = [others[0], others[-1]]
    for pos in range(3):
        group = [CastRun(*others[0], ct), CastRun(*others[1], ct)]
        mine = CastRun(R, Cn, ct)
        group.insert(pos, mine)
        cast_launch(group)
        for key, a in alone.outputs().items():
            assert torch.equal(a, mine.outputs()[key]), f"rows_cast_ws {R}x{Cn} at position {pos} of three: {key} differs from the launch alone"
        group[0 if pos else 1].check(f"rows_cast_ws, a neighbour of {R}x{Cn} at position {pos}")


def test_rows_cast_ws_problems_that_share_colsum():
    first = None
    for k in range(10):
        a, b = CastRun(129, 37, False), CastRun(33, 37, False)
        b.p.colsum = a.p.colsum
        cast_launch([a, b])
        if first is None:
            first = bits(a.cs.buf)
            close(a.cs.v, a.r.s_cs.double() + a.r.a.double().sum(0) + b.r.a.double().sum(0), 1e-4, "shared colsum")
        assert torch.equal(first, bits(a.cs.buf)), f"shared colsum: launch {k} differs from launch 0"
