"""The HIP criterion (csrc/loss.hip, losses.py) against torch's functional in fp64 on the CPU.

Error measure: max |got - ref| over the tensor / max(max |ref|, tiny) -- for a scalar loss the relative error.
Tolerance: what torch's OWN fp32 criterion (forward and autograd backward, same device, same inputs) shows in that
measure against the fp64 value, times 2 -- measured inside each test -- with a floor of 4 * 2^-24 where torch happens to
be exact (the pattern of tests/test_gelu_gpu.py).  The kernels carry every element in fp64 and round once (2^-24), the
backward multiplies two fp32 values (one more rounding): both fit under the floor, so the floor usually rules.
No tolerance here comes from what the HIP path gives; tools/loss_errors.py records both sides in
profiles/loss_errors.json.
"""
import functools
from types import SimpleNamespace

import numpy as np
import pytest
import torch
import torch.nn.functional as F

pytestmark = pytest.mark.gpu

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import _lib, losses, ops, training  # noqa: E402

DEV = "cuda"
NAN = float("nan")
ULP = 2.0 ** -24
TINY = 1e-30
G = 64                         # guard elements on either side of a view (256 bytes: keeps the view's alignment)
KINDS = {"bce": _lib.LOSS_BCE, "ce": _lib.LOSS_CE, "l1": _lib.LOSS_L1}
REDS = {"mean": _lib.LOSS_MEAN, "sum": _lib.LOSS_SUM, "none": _lib.LOSS_NONE}
# the degenerate case; the headline's shape (C % 4 != 0); more rows than columns; past one workgroup (30300 elements, 300
# row blocks); a row past one wave's pass and past one block's (5000 > 256 columns per pass)
SHAPES = [(1, 1), (8, 23), (33, 4), (300, 101), (4, 5000)]
IGNORE = -100


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

    def check_pad(self, cols, what):
        """columns [cols, ld) of every row hold what they held before the launch"""
        lo, n = self.lo, self.n
        got, was = bits(self.buf)[lo:lo + n].view(self.v.shape), bits(self.init)[lo:lo + n].view(self.v.shape)
        assert torch.equal(got[:, cols:], was[:, cols:]), what + ": pad columns were written"


def rel_err(got, ref):
    got, ref = got.detach().double().cpu(), ref.detach().double().cpu()
    assert got.shape == ref.shape, (got.shape, ref.shape)
    assert torch.isfinite(got).all(), "non-finite value"
    return float((got - ref).abs().max() / max(float(ref.abs().max()), TINY)) if ref.numel() else 0.0


def tol_of(e_torch):
    return 2 * max(e_torch, 4 * ULP)


def functional(kind, x, y, w, red, ignore=IGNORE):
    if kind == "bce":
        return F.binary_cross_entropy_with_logits(x, y, pos_weight=w, reduction=red)
    if kind == "ce":
        return F.cross_entropy(x, y, weight=w, ignore_index=ignore, reduction=red)
    return F.l1_loss(x, y, reduction=red)


def loss_and_grad(kind, x, y, w, red, up=None):
    """(loss, d/dx of sum(loss * up)) by torch's functional + autograd, in x's dtype and on x's device"""
    x = x.detach().clone().requires_grad_(True)
    l = functional(kind, x, y, w, red)
    ((l if up is None else l * up).sum()).backward()
    return l.detach(), x.grad.detach()


@functools.lru_cache(maxsize=None)
def data(kind, B, Cn, weighted):
    """Host inputs (fp32 values) and the fp64 references of the three reductions; never modified."""
    g = torch.Generator().manual_seed(1000 * B + Cn + 7 * len(kind) + weighted)
    x = 3 * torch.randn(B, Cn, generator=g)
    if kind == "ce":
        y = torch.randint(0, Cn, (B,), generator=g)
        if B >= 8:
            y[1::5] = IGNORE
    elif kind == "bce":
        y = torch.rand(B, Cn, generator=g)
        y[torch.rand(B, Cn, generator=g) < 0.5] = 1.0          # hard and soft targets
        y[torch.rand(B, Cn, generator=g) < 0.3] = 0.0
    else:
        y = torch.randn(B, Cn, generator=g)
    w = (0.25 + 8 * torch.rand(Cn, generator=g)) if weighted else None
    r = SimpleNamespace(x=x, y=y, w=w, ref={})
    y64, w64 = (y if kind == "ce" else y.double()), (None if w is None else w.double())
    for red in REDS:
        r.ref[red] = loss_and_grad(kind, x.double(), y64, w64, red)
    return r


def torch_f32_errors(kind, d, red, up=None, ref=None):
    l, gx = loss_and_grad(kind, d.x.to(DEV), d.y.to(DEV), None if d.w is None else d.w.to(DEV), red,
                          None if up is None else up.to(DEV))
    ref = ref or d.ref[red]
    return rel_err(l, ref[0]), rel_err(gx, ref[1])


CASES = [(k, r, s, w) for k in KINDS for r in REDS for s in SHAPES for w in (False, True) if not (k == "l1" and w)]


@pytest.mark.parametrize("kind,red,shape,weighted", CASES, ids=[f"{k}-{r}-{s[0]}x{s[1]}-{'w' if w else 'nw'}" for k, r, s, w in CASES])
def test_kernels_against_fp64(kind, red, shape, weighted):
    """Through the C ABI, with padded leading dimensions inside sentinel-guarded buffers: loss and dlogits_unit against
    fp64, dlogits = dlogits_unit * g with g = 1 read on the device, pad columns and guard words untouched."""
    B, Cn = shape
    d = data(kind, B, Cn, weighted)
    e_l, e_g = torch_f32_errors(kind, d, red)
    print(f"torch fp32 {kind} {red} {shape}: loss err {e_l:.3e}, grad err {e_g:.3e}")
    ld, ldt, ldd, lddl, ldg = Cn + 3, Cn + 2, Cn + 5, Cn + 1, Cn + 4
    x = Guarded(B, ld, skew=1)                              # pad columns hold NaN
    x.v[:, :Cn] = d.x.to(DEV)
    x.init = x.buf.clone()
    if kind == "ce":
        yg, y, ldt = None, d.y.to(DEV), None
    else:
        yg = Guarded(B, ldt, skew=3)                        # pad columns hold NaN
        yg.v[:, :Cn] = d.y.to(DEV)
        yg.init = yg.buf.clone()
        y = yg.v
    w = None if d.w is None else d.w.to(DEV)
    loss_shape = (1,) if red != "none" else (B,) if kind == "ce" else (B, Cn)
    loss = Guarded(*loss_shape, skew=2)
    du, dl = Guarded(B, ldd, skew=1), Guarded(B, lddl, skew=2)
    nws = ops.loss_ws_bytes(KINDS[kind], REDS[red], B, Cn)
    ws = Guarded(nws // 4 + 2, fill=NAN) if nws else None      # (byte offset 256 of the buffer: 8-byte aligned)
    bad = torch.zeros(1, device=DEV, dtype=torch.int32)
    prob = ops.loss_problem(KINDS[kind], REDS[red], x.v, y, loss.v, B, Cn, ld=ld, ldt=ldt, weight=w, ignore_index=IGNORE,
                            dlogits_unit=du.v, ldd=ldd, bad=bad if kind == "ce" else None, ws=None if ws is None else ws.v)
    ops.loss_fwd(prob)
    if red != "none":
        gup = Guarded(1, fill=1.0)
    elif kind == "ce":
        gup = Guarded(B, fill=1.0)
    else:
        gup = Guarded(B, ldg, fill=NAN)                     # pad columns of the upstream gradient hold NaN
        gup.v[:, :Cn] = 1.0
    ops.loss_bwd(prob, gup.v, dl.v, ldg=ldg, lddl=lddl)
    torch.cuda.synchronize()
    what = f"{kind} {red} {shape}"
    for t in (x, loss, du, dl) + ((ws,) if ws is not None else ()):
        t.check(what)
    du.check_pad(Cn, what + " dlogits_unit")
    dl.check_pad(Cn, what + " dlogits")
    assert torch.equal(bits(x.buf), bits(x.init)), "the logits were written"
    assert yg is None or torch.equal(bits(yg.buf), bits(yg.init)), "the targets were written"
    ref_l, ref_g = d.ref[red]
    got_l = loss.v.view(ref_l.shape)
    a_l, a_g = rel_err(got_l, ref_l), rel_err(du.v[:, :Cn], ref_g)
    print(f"hip {what}: loss err {a_l:.3e}, grad err {a_g:.3e}")
    assert a_l <= tol_of(e_l), (a_l, tol_of(e_l))
    assert a_g <= tol_of(e_g), (a_g, tol_of(e_g))
    assert torch.equal(bits(dl.v[:, :Cn]), bits(du.v[:, :Cn])), "dlogits != dlogits_unit * 1"
    assert int(bad) == 0


# ---------------------------------------------------------------------------------------------------------------------
# modules
# ---------------------------------------------------------------------------------------------------------------------
def run_module(crit, x, y, up=None, div=None):
    """loss and d/dx through the module on the device; up: weights of the `none` elements, div: loss / div"""
    xd = x.to(DEV).requires_grad_(True)
    l = crit.to(DEV)(xd, y.to(DEV))
    out = l if up is None else l * up.to(DEV)
    (out.sum() if div is None else out.sum() / div).backward()
    return l.detach(), xd.grad.detach()


def module_for(kind, w, red, hip=True, ignore=IGNORE):
    mod = losses if hip else torch.nn
    if kind == "bce":
        return mod.BCEWithLogitsLoss(pos_weight=w, reduction=red)
    if kind == "ce":
        return mod.CrossEntropyLoss(weight=w, ignore_index=ignore, reduction=red)
    return mod.L1Loss(reduction=red)


def compare(kind, x, y, w, red, up=None, div=None, ignore=IGNORE):
    """HIP module against fp64, bounded by twice torch's own fp32 error on the device"""
    def ref_run(xx, yy, ww, uu):
        xx = xx.detach().clone().requires_grad_(True)
        l = functional(kind, xx, yy, ww, red, ignore)
        out = (l if uu is None else l * uu).sum()
        (out if div is None else out / div).backward()
        return l.detach(), xx.grad.detach()
    y64 = y if kind == "ce" else y.double()
    ref = ref_run(x.double(), y64, None if w is None else w.double(), None if up is None else up.double())
    t32 = ref_run(x.to(DEV), y.to(DEV), None if w is None else w.to(DEV), None if up is None else up.to(DEV))
    got = run_module(module_for(kind, w, red, ignore=ignore), x, y, up, div)
    for i, name in enumerate(("loss", "grad")):
        e_t, e_h = rel_err(t32[i], ref[i]), rel_err(got[i], ref[i])
        print(f"{kind} {red} {name}: torch fp32 err {e_t:.3e}, hip err {e_h:.3e}")
        assert e_h <= tol_of(e_t), (kind, red, name, e_h, tol_of(e_t))
    return got, ref


@pytest.mark.parametrize("red", list(REDS))
@pytest.mark.parametrize("weighted", [False, True])
def test_bce_special_values(red, weighted):
    xs = torch.tensor([0., 17., -17., 90., -90., 1e4, -1e4])
    ys = torch.tensor([0., 1., 0.25])
    x = xs[:, None].expand(7, 3).contiguous()
    y = ys[None, :].expand(7, 3).contiguous()
    w = torch.tensor([50., 0.5, 7.]) if weighted else None
    (l, gx), _ = compare("bce", x, y, w, red)
    assert torch.isfinite(l).all() and torch.isfinite(gx).all()


@pytest.mark.parametrize("red", list(REDS))
def test_ce_rows_shifted_by_1e4(red):
    g = torch.Generator().manual_seed(11)
    x = torch.randn(9, 5, generator=g) + 1e4
    y = torch.randint(0, 5, (9,), generator=g)
    (l, gx), _ = compare("ce", x, y, 0.5 + torch.rand(5, generator=g), red)
    assert torch.isfinite(l).all() and torch.isfinite(gx).all()


def test_ce_saturated_row_is_exactly_zero():
    g = torch.Generator().manual_seed(12)
    x = torch.randn(6, 9, generator=g)
    y = torch.randint(0, 9, (6,), generator=g)
    x[2, 4] = x[2].max() + 200.0
    y[2] = 4
    for red in REDS:
        l, gx = run_module(losses.CrossEntropyLoss(reduction=red), x, y)
        assert torch.equal(bits(gx[2]), torch.zeros(9, dtype=torch.int32)), red     # +0.0 bits in every column
        assert float(gx[1].abs().max()) > 0
        if red == "none":
            assert torch.equal(bits(l[2:3]), torch.zeros(1, dtype=torch.int32))


@pytest.mark.parametrize("red", list(REDS))
def test_ce_ignored_rows_and_a_zero_class_weight(red):
    g = torch.Generator().manual_seed(13)
    x = 2 * torch.randn(9, 5, generator=g)
    y = torch.tensor([0, 1, IGNORE, 2, 3, IGNORE, 4, 1, 2])
    w = torch.tensor([1.5, 0.0, 2.0, 0.25, 3.0])            # rows 1 and 7 are kept with weight 0
    (l, gx), _ = compare("ce", x, y, w, red)
    for row in (2, 5, 1, 7):
        assert float(gx[row].abs().max()) == 0.0
    assert float(gx[0].abs().max()) > 0
    crit = losses.CrossEntropyLoss(weight=w, reduction=red)
    run_module(crit, x, y)
    assert int(crit.bad_targets) == 0                       # ignore_index itself lies outside [0, C): not a bad target


def test_ce_all_rows_ignored():
    x = torch.randn(5, 4, generator=torch.Generator().manual_seed(14))
    y = torch.full((5,), IGNORE)
    for w in (None, torch.tensor([1., 2., 3., 4.])):
        ref_mean = F.cross_entropy(x.double(), y, weight=None if w is None else w.double())
        assert torch.isnan(ref_mean)                        # torch's own answer
        xd = x.to(DEV).requires_grad_(True)
        l = losses.CrossEntropyLoss(weight=w).to(DEV)(xd, y.to(DEV))
        assert torch.isnan(l)
        l, gx = run_module(losses.CrossEntropyLoss(weight=w, reduction="sum"), x, y)
        assert torch.equal(bits(l.view(1)), torch.zeros(1, dtype=torch.int32))
        assert torch.equal(bits(gx), torch.zeros(5, 4, dtype=torch.int32))
        l, gx = run_module(losses.CrossEntropyLoss(weight=w, reduction="none"), x, y)
        assert torch.equal(bits(l), torch.zeros(5, dtype=torch.int32)) and torch.equal(bits(gx), torch.zeros(5, 4, dtype=torch.int32))
    # kept rows whose total weight is 0: NaN as well
    w0 = torch.tensor([0., 0., 1., 1.])
    y0 = torch.tensor([0, 1, 1, IGNORE, 0])
    assert torch.isnan(F.cross_entropy(x.double(), y0, weight=w0.double()))
    l, _ = run_module(losses.CrossEntropyLoss(weight=w0), x, y0)
    assert torch.isnan(l)
    l, _ = run_module(losses.CrossEntropyLoss(weight=w0, reduction="sum"), x, y0)
    assert float(l) == 0.0


@pytest.mark.parametrize("shape", [(8, 23), (5,), (3, 7, 11)])
def test_l1_gradient_is_the_sign_times_one_over_n(shape):
    g = torch.Generator().manual_seed(15)
    x = torch.randn(*shape, generator=g)
    y = torch.randn(*shape, generator=g)
    y.view(-1)[::3] = x.view(-1)[::3]                       # x == y: gradient exactly 0
    n = x.numel()
    for red, scale in (("mean", torch.tensor(1.0 / n, dtype=torch.float32)), ("sum", torch.tensor(1.0)), ("none", torch.tensor(1.0))):
        l, gx = run_module(losses.L1Loss(reduction=red), x, y)
        want = torch.sign(x - y) * scale
        assert torch.equal(bits(gx) & 0x7FFFFFFF, bits(want) & 0x7FFFFFFF), red     # magnitudes bit-equal
        assert torch.equal(torch.sign(gx.cpu()), torch.sign(want)), red             # and the signs (0 where x == y)
        assert l.shape == (x.shape if red == "none" else ())
        ref = F.l1_loss(x.double(), y.double(), reduction=red)
        e_t = rel_err(F.l1_loss(x.to(DEV), y.to(DEV), reduction=red), ref)
        assert rel_err(l, ref) <= tol_of(e_t)


# ---------------------------------------------------------------------------------------------------------------------
# upstream gradients
# ---------------------------------------------------------------------------------------------------------------------
@pytest.mark.parametrize("weighted", [False, True])
@pytest.mark.parametrize("kind", list(KINDS))
def test_upstream_gradients(kind, weighted):
    if kind == "l1" and weighted:
        weighted = False
    d = data(kind, 33, 4, weighted)
    g = torch.Generator().manual_seed(16)
    for red in ("mean", "sum"):
        compare(kind, d.x, d.y, d.w, red, div=4)            # (loss / 4).backward()
    up = torch.randn(33, generator=g) if kind == "ce" else torch.randn(33, 4, generator=g)
    compare(kind, d.x, d.y, d.w, "none", up=up)             # (loss_none * r).sum().backward()


@pytest.mark.parametrize("kind", list(KINDS))
def test_no_gradient_buffer_without_a_gradient_request(kind, monkeypatch):
    d = data(kind, 8, 23, kind != "l1")
    seen = []
    real = ops.loss_problem

    def spy(*a, **kw):
        seen.append(kw.get("dlogits_unit"))
        return real(*a, **kw)

    monkeypatch.setattr(ops, "loss_problem", spy)
    for red in REDS:
        crit = module_for(kind, d.w, red).to(DEV)
        x, y = d.x.to(DEV), d.y.to(DEV)
        del seen[:]
        with_grad = crit(x.clone().requires_grad_(True), y)
        with torch.no_grad():
            under_no_grad = crit(x.clone().requires_grad_(True), y)
        plain = crit(x, y)
        assert seen[0] is not None and seen[0].shape == (8, 23) and seen[1] is None and seen[2] is None
        assert with_grad.requires_grad and not under_no_grad.requires_grad and not plain.requires_grad
        assert torch.equal(bits(with_grad), bits(under_no_grad)) and torch.equal(bits(with_grad), bits(plain))


@pytest.mark.parametrize("shape", [(300, 101), (4, 5000)])
@pytest.mark.parametrize("kind", list(KINDS))
def test_two_runs_give_identical_bits(kind, shape):
    d = data(kind, shape[0], shape[1], kind != "l1")
    for red in ("mean", "none"):
        up = None if red == "mean" else (torch.ones(shape[0]) if kind == "ce" else torch.ones(*shape)) * 0.37
        a = run_module(module_for(kind, d.w, red), d.x, d.y, up)
        b = run_module(module_for(kind, d.w, red), d.x, d.y, up)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1]))


def test_other_dtypes_shapes_and_strides():
    """bf16 / fp64 inputs are cast to fp32 (the loss comes back in the input's dtype); BCE / L1 flatten any equal shapes;
    a column-strided input is made contiguous, a row-strided one is read in place.  Bound: the floor of tol_of (the
    kernel's one rounding per element and the backward's product stay under it)."""
    g = torch.Generator().manual_seed(17)
    x, y = torch.randn(6, 10, generator=g), torch.rand(6, 10, generator=g)
    ref_l, ref_g = loss_and_grad("bce", x.double(), y.double(), None, "mean")
    for dt in (torch.bfloat16, torch.float64):
        xd = x.to(DEV).to(dt).requires_grad_(True)
        l = losses.BCEWithLogitsLoss()(xd, y.to(DEV).to(dt))
        l.backward()
        assert l.dtype == dt and xd.grad.dtype == dt
        if dt == torch.float64:
            assert rel_err(l, ref_l) <= tol_of(0) and rel_err(xd.grad, ref_g) <= tol_of(0)
    big = torch.randn(6, 20, generator=g).to(DEV)
    for view in (big[:, :10], big[:, ::2]):
        xv = view.detach().requires_grad_(True)
        l = losses.BCEWithLogitsLoss()(xv, y.to(DEV))
        l.backward()
        r_l, r_g = loss_and_grad("bce", view.double().cpu(), y.double(), None, "mean")
        assert rel_err(l, r_l) <= tol_of(0) and rel_err(xv.grad, r_g) <= tol_of(0)
    x3, y3 = torch.randn(2, 3, 5, generator=g), torch.rand(2, 3, 5, generator=g)
    w = torch.rand(5, generator=g) + 0.5
    l, gx = run_module(losses.BCEWithLogitsLoss(pos_weight=w, reduction="none"), x3, y3)
    r_l, r_g = loss_and_grad("bce", x3.double(), y3.double(), w.double(), "none")
    assert l.shape == (2, 3, 5) and rel_err(l, r_l) <= tol_of(0) and rel_err(gx, r_g) <= tol_of(0)
    t = torch.randint(0, 10, (6,), generator=g, dtype=torch.int32)          # int32 class indices are widened
    l, gx = run_module(losses.CrossEntropyLoss(), x, t)
    r_l, r_g = loss_and_grad("ce", x.double(), t.long(), None, "mean")
    assert rel_err(l, r_l) <= tol_of(0) and rel_err(gx, r_g) <= tol_of(0)


# ---------------------------------------------------------------------------------------------------------------------
# class indices outside [0, C)
# ---------------------------------------------------------------------------------------------------------------------
def test_out_of_range_class_indices_are_counted_and_ignored():
    """Defined behaviour of the entry: the index is compared with [0, C) before it is used, the row is treated as ignored."""
    Cn = 7
    g = torch.Generator().manual_seed(18)
    x = torch.randn(12, Cn, generator=g)
    y = torch.randint(0, Cn, (12,), generator=g)
    y[9] = IGNORE
    y_bad, y_ign = y.clone(), y.clone()
    y_bad[2], y_bad[5], y_bad[10] = Cn, -1, 2 ** 40
    y_ign[2] = y_ign[5] = y_ign[10] = IGNORE
    w = 0.5 + torch.rand(Cn, generator=g)
    crit_bad = losses.CrossEntropyLoss(weight=w)
    crit_ign = losses.CrossEntropyLoss(weight=w)
    for i, red in enumerate(REDS):
        crit_bad.reduction = crit_ign.reduction = red
        a = run_module(crit_bad, x, y_bad)
        b = run_module(crit_ign, x, y_ign)
        assert torch.equal(bits(a[0]), bits(b[0])) and torch.equal(bits(a[1]), bits(b[1])), red
        assert torch.isfinite(a[0]).all() and float(a[1][2].abs().max()) == 0.0
        assert crit_bad.bad_targets.dtype == torch.int32 and crit_bad.bad_targets.is_cuda
        assert int(crit_bad.bad_targets) == 3 * (i + 1)     # cumulative
        assert int(crit_ign.bad_targets) == 0
    ref_l, ref_g = loss_and_grad("ce", x.double(), y_ign, w.double(), "none")
    assert rel_err(a[0], ref_l) <= tol_of(0) and rel_err(a[1], ref_g) <= tol_of(0)


# ---------------------------------------------------------------------------------------------------------------------
# through a model
# ---------------------------------------------------------------------------------------------------------------------
def _model_args(**kw):
    a = dict(model="mmtrvat", orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=24, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=1, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0., res_dropout=0.,
             out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6, bert_model="unused", text_features=True,
             num_vectors_l=32, num_vectors_a=32, num_vectors_v=32, precision="f32")
    a.update(kw)
    return SimpleNamespace(**a)


def test_through_a_model_and_one_training_step():
    from bpmult_amd.models import get_model
    from bpmult_amd.optim import FusedAdam
    torch.manual_seed(19)
    args = _model_args(task_type="multilabel", task="mmimdb", weight_classes=1, labels=list("abcdef"),
                       label_freqs=dict(zip("abcdef", (900, 400, 120, 60, 33, 700))), train_data_len=1500, criterion="hip")
    model = get_model(args).cuda().eval()
    opt = FusedAdam(model, lr=1e-2)
    g = torch.Generator().manual_seed(20)
    txt, img, aud = torch.randn(2, 10, 32, generator=g), torch.randn(2, 20, 35, generator=g), torch.randn(2, 30, 74, generator=g)
    tgt = (torch.rand(2, 6, generator=g) > 0.5).float()
    crit = training.get_criterion(args).to(DEV)
    assert type(crit) is losses.BCEWithLogitsLoss and crit.pos_weight.is_cuda
    logits = model(txt.cuda(), None, None, img.cuda(), aud.cuda())
    logits.retain_grad()
    loss_h = crit(logits, tgt.cuda())
    loss_h.backward()
    w = crit.pos_weight.detach().cpu()
    vals = logits.detach().cpu()
    ref_l, ref_g = loss_and_grad("bce", vals.double(), tgt.double(), w.double(), "mean")
    t_l, t_g = loss_and_grad("bce", vals.to(DEV), tgt.to(DEV), w.to(DEV), "mean")       # torch's, on the same logits values
    for name, got, t32, ref in (("loss", loss_h, t_l, ref_l), ("logits.grad", logits.grad, t_g, ref_g)):
        e_t, e_h = rel_err(t32, ref), rel_err(got, ref)
        print(f"model {name}: torch fp32 err {e_t:.3e}, hip err {e_h:.3e}")
        assert e_h <= tol_of(e_t), (name, e_h, tol_of(e_t))
    assert all(p.grad is None or torch.isfinite(p.grad).all() for p in model.parameters())
    # one step of the reference's loop with the HIP criterion: model_forward + backward + FusedAdam
    model.train()
    opt.zero_grad()
    before = {k: p.detach().clone() for k, p in model.named_parameters()}
    zeros = torch.zeros(2, 10, dtype=torch.long)
    loss, out, t = training.model_forward(model, crit, (txt, zeros, zeros, img, tgt, aud), "mmtrvat")
    assert out.shape == (2, 6) and loss.dim() == 0 and torch.isfinite(loss)
    loss.backward()
    opt.step()
    torch.cuda.synchronize()
    after = dict(model.named_parameters())
    assert all(torch.isfinite(p).all() for p in after.values())
    moved = [k for k in after if not torch.equal(after[k].detach(), before[k])]
    assert any(k.startswith("trans_") for k in moved) and "out_layer.weight" in moved, moved[:5]
