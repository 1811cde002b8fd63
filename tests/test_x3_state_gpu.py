"""The bf16x3 split-image cache (ops._X3Plan, _X3_BUFFERS, _X3_STATIC_SPLITS, _X3_FRESH / _X3_EPOCH, x3_presplit) through
ops.gemm_grouped(..., x3=True), without a model.  An operand's [hi | lo] bf16 image is cached per (address, rows, cols, ld);
a weight's image is refreshed only by x3_refresh_static(), an activation's is skipped when an earlier launch of the same
step left it, and that decision is frozen when the launch's plan is built.  A stale image gives finite, plausible numbers:
every result here is compared with the fp64 product of the fp32 operands AS THEY ARE IN MEMORY WHEN THE LAUNCH RUNS, at the
bf16x3 limit of tests/test_kernels_gpu.py::test_gemm_bf16x3_products (5e-5 of the result's scale); rewritten operands are
fresh draws, so a stale image is off by the scale itself.

Launch sizes: NT / NN three problems of 256 x 256 x 256 (as test_gemm_bf16x3_products pads its launches); TN 24 problems of
512 x 512 x 256 = 96 tiles of 256 x 256, the least a weight-gradient launch needs for the split path."""
import pytest
import torch

pytestmark = pytest.mark.gpu

from test_kernels_gpu import rnd  # noqa: E402

from bpmult_amd import ops  # noqa: E402
from bpmult_amd.ops import BPM_F32, GEMM_NN, GEMM_NT, GEMM_TN  # noqa: E402

DEV = "cuda"
X3_TOL = 5e-5
NAMES = {GEMM_NT: "nt", GEMM_NN: "nn", GEMM_TN: "tn"}
_seed = [100]


def fresh(*shape, scale=1.0):
    """A new draw every call (CPU fp32)."""
    _seed[0] += 1
    return rnd(*shape, seed=_seed[0], scale=scale)


def product(variant, a, b):
    a, b = a.detach().cpu().double(), b.detach().cpu().double()
    return a @ b.T if variant == GEMM_NT else (a @ b if variant == GEMM_NN else a.T @ b)


def operand_shapes(variant, M, N, K):
    return ((M, K) if variant != GEMM_TN else (K, M)), ((N, K) if variant == GEMM_NT else (K, N))


class Launch:
    """One grouped launch over (A, B) operand pairs (device fp32 tensors, or (tensor, rows, cols, ld) views of one); its
    problem array is built once and replayed, like a launch table of the engine."""

    def __init__(self, variant, pairs, presplit=()):
        self.variant, self.pairs, self.outs, probs = variant, pairs, [], []
        for a, b in pairs:
            (ta, ra, ca, lda), (tb, rb, cb, ldb) = self._view(a), self._view(b)
            if variant == GEMM_NT:
                M, K, N = ra, ca, rb
            elif variant == GEMM_NN:
                M, K, N = ra, ca, cb
            else:
                K, M, N = ra, ca, cb
            out = torch.full((M, N), float("nan"), device=DEV)
            self.outs.append(out)
            probs.append(ops.gemm_problem(ta, tb, out, M, N, K, lda, ldb, N, flags=ops.F_KPAD))
        self.arr = ops.array(ops.GemmProblem, probs)
        if presplit:
            self.arr.x3_presplit = frozenset(t.data_ptr() for t in presplit)

    @staticmethod
    def _view(t):
        return t if isinstance(t, tuple) else (t, t.shape[0], t.shape[1], t.shape[1])

    @staticmethod
    def _values(v):
        t, rows, cols, ld = Launch._view(v)
        return t.detach().cpu().reshape(-1)[:rows * ld].view(rows, ld)[:, :cols]

    def run(self):
        for o in self.outs:
            o.fill_(float("nan"))
        ops.gemm_grouped(BPM_F32, self.variant, self.arr, x3=True)
        assert self.arr._x3_plan.ok, "this launch must take the split-bf16 path, not the exact fp32 fallback"

    def errors(self, operands=None):
        """max |out - fp64 product| / scale per problem, against the operands in memory now (or the given values)."""
        refs, errs = {}, []
        for i, ((a, b), out) in enumerate(zip(self.pairs, self.outs)):
            k = (id(a), id(b))
            if k not in refs:
                va, vb = operands[i] if operands is not None else (self._values(a), self._values(b))
                refs[k] = product(self.variant, va, vb)
            ref = refs[k]
            got = out.cpu().double()
            assert torch.isfinite(got).all(), f"problem {i}: non-finite output"
            errs.append(float((got - ref).abs().max()) / float(ref.abs().max()))
        return errs

    def check(self, what):
        errs = self.errors()
        worst = max(errs)
        assert worst <= X3_TOL, f"{what} ({NAMES[self.variant]}): max err / scale = {worst:.2e} (problem {errs.index(worst)})"


def plain_launch(variant, shared=None, side="A"):
    """NT / NN: three problems of 256^3; TN: 24 of 512 x 512 x 256 over two A operands.  `shared`: the operand under test,
    used on `side` of every problem (otherwise every problem has operands of its own)."""
    if variant == GEMM_TN:
        G, (sa, sb) = 24, operand_shapes(variant, 512, 512, 256)
        pool = [fresh(*(sb if side == "A" else sa), scale=1.0 if side == "B" else 256 ** -0.5).to(DEV) for _ in range(2)]
    else:
        G, (sa, sb) = 3, operand_shapes(variant, 256, 256, 256)
        pool = [fresh(*(sb if side == "A" else sa), scale=1.0 if side == "B" else 256 ** -0.5).to(DEV) for _ in range(G)]
    if shared is None:
        shared_of = [fresh(*(sa if side == "A" else sb)).to(DEV) for _ in range(len(pool))]
    else:
        assert tuple(shared.shape) == (sa if side == "A" else sb)
        shared_of = [shared] * len(pool)
    pairs = [((shared_of[i % len(pool)], pool[i % len(pool)]) if side == "A" else (pool[i % len(pool)], shared_of[i % len(pool)]))
             for i in range(G)]
    return Launch(variant, pairs)


@pytest.mark.parametrize("variant", [GEMM_NT, GEMM_NN, GEMM_TN], ids=NAMES.get)
def test_dynamic_operand_rewritten_in_place(variant):
    """The same problem array launched twice with both operands rewritten in place in between: the second result follows the
    new values (an activation buffer of the hot path: same address every step, new contents)."""
    L = plain_launch(variant)
    L.run()
    L.check("first launch")
    for a, b in {(id(a), id(b)): (a, b) for a, b in L.pairs}.values():
        a.copy_(fresh(*a.shape))
        b.copy_(fresh(*b.shape, scale=256 ** -0.5))
    L.run()
    L.check("after the operands were rewritten in place")


@pytest.mark.parametrize("variant", [GEMM_NT, GEMM_NN], ids=NAMES.get)
def test_static_range_follows_refresh_and_drop(variant):
    """A weight buffer inside a registered static range (ParamStore.finalize_shadows): split when a plan first meets it, again
    only by x3_refresh_static() (ParamStore.refresh_shadows) -- after which the result follows the new weights -- and, once
    the range is dropped (x3_drop_static: the store is gone), split on every launch of a new table like any other operand."""
    _, sb = operand_shapes(variant, 256, 256, 256)
    W = fresh(*sb, scale=256 ** -0.5).to(DEV)                # the B operand of the forward (NT) and data-gradient (NN) products
    lo = W.data_ptr()
    rng = (lo, lo + W.numel() * W.element_size())
    try:
        ops.x3_register_static(*rng)
        L = plain_launch(variant, shared=W, side="B")
        L.run()
        L.check("first launch over the static range")
        assert any(k[0] == lo for k in ops._X3_STATIC_SPLITS), "the weight buffer was taken as a static operand"
        old = W.cpu().clone()
        W.copy_(fresh(*sb, scale=256 ** -0.5))
        L.run()                                              # no refresh yet: the image is the old weights' (that is the
        stale = L.errors([(Launch._values(a), old) for a, _ in L.pairs])      # caching this file is about -- it is real)
        assert max(stale) <= X3_TOL, f"before x3_refresh_static() the launch still reads the image of the old weights: {max(stale):.2e}"
        ops.x3_refresh_static()
        L.run()
        L.check("after the weights were rewritten and x3_refresh_static()")
        ops.x3_drop_static(*rng)
        assert not any(k[0] == lo for k in ops._X3_STATIC_SPLITS) and rng not in ops._X3_STATIC
        L2 = plain_launch(variant, shared=W, side="B")       # a new launch table over the same address
        L2.run()
        L2.check("first launch after x3_drop_static")
        W.copy_(fresh(*sb, scale=256 ** -0.5))
        L2.run()                                             # no refresh: a dynamic operand is split by every launch
        L2.check("rewritten after x3_drop_static, no refresh")
        assert not any(k[0] == lo for k in ops._X3_STATIC_SPLITS)
    finally:
        ops.x3_drop_static(*rng)


def _presplit_pair():
    """Launch 1 (NT, a forward product) splits the activation X [256, 512]; launch 2 (TN, the weight gradient that reads X
    again as its B operand: the same (address, rows, cols, ld)) is tagged x3_presplit = {X}."""
    X = fresh(256, 512).to(DEV)
    Ws = [fresh(256, 512, scale=512 ** -0.5).to(DEV) for _ in range(3)]
    L1 = Launch(GEMM_NT, [(X, w) for w in Ws])
    dY = [fresh(256, 512, scale=256 ** -0.5).to(DEV) for _ in range(2)]
    L2 = Launch(GEMM_TN, [(dY[i % 2], X) for i in range(24)], presplit=(X,))
    return X, L1, L2


def test_presplit_image_is_reused_within_a_step_and_renewed_in_the_next():
    X, L1, L2 = _presplit_pair()
    ops.x3_new_step()
    L1.run()
    L2.run()                                                 # its plan is built now, in the step of launch 1's split
    L1.check("launch 1")
    L2.check("launch 2 (x3_presplit) in the step of launch 1")
    # the reuse is real: launch 2 alone, after X changed, still reads the image launch 1 left (in the engine launch 1 always
    # runs first; this only shows that the path under test is the presplit one)
    old = X.cpu().clone()
    X.copy_(fresh(256, 512))
    L2.run()
    stale = L2.errors([(Launch._values(a), old) for a, _ in L2.pairs])
    assert max(stale) <= X3_TOL, f"launch 2 is expected to reuse launch 1's image of X: {max(stale):.2e}"
    for step in range(2):
        ops.x3_new_step()
        X.copy_(fresh(256, 512))
        L1.run()
        L2.run()
        L1.check(f"launch 1, step {step + 1}")
        L2.check(f"launch 2 (x3_presplit), step {step + 1}: X was rewritten")


def test_presplit_across_two_streams_ordered_by_an_event():
    """As the engine runs its weight gradients: launch 1 on the main stream, launch 2 on a side stream behind an event."""
    X, L1, L2 = _presplit_pair()
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()

    def step():
        ops.x3_new_step()
        L1.run()
        ev = torch.cuda.Event()
        ev.record(main)
        side.wait_event(ev)
        with torch.cuda.stream(side):
            L2.run()
        main.wait_stream(side)

    step()
    L1.check("launch 1")
    L2.check("launch 2 on the side stream")
    for k in range(2):
        X.copy_(fresh(256, 512))
        step()
        L1.check(f"launch 1, step {k + 1}")
        L2.check(f"launch 2 on the side stream, step {k + 1}: X was rewritten")


@pytest.mark.parametrize("variant", [GEMM_NT, GEMM_TN], ids=NAMES.get)
def test_address_reuse_by_the_caching_allocator(variant, capsys):
    """Images are keyed by raw address: an operand is freed and another tensor of the same shape allocated.  When the
    allocator hands out the same address (it does for a same-size block), the result must use the new contents."""
    side = "A" if variant == GEMM_NT else "B"
    sa, sb = operand_shapes(variant, *((256, 256, 256) if variant == GEMM_NT else (512, 512, 256)))
    shape = sa if side == "A" else sb
    X1 = fresh(*shape).to(DEV)
    ptr = X1.data_ptr()
    L = plain_launch(variant, shared=X1, side=side)
    L.run()
    L.check("first tensor")
    torch.cuda.synchronize()
    del L, X1
    X2 = torch.empty(*shape, device=DEV)
    X2.copy_(fresh(*shape))
    same = X2.data_ptr() == ptr
    with capsys.disabled():
        print(f"\n[x3 address reuse, {NAMES[variant]}] the allocator returned {'the SAME address' if same else 'ANOTHER address'}")
    L = plain_launch(variant, shared=X2, side=side)
    L.run()
    L.check("second tensor" + (" at the first one's address" if same else ""))
    X2.copy_(fresh(*shape))
    L.run()
    L.check("second tensor rewritten")


def test_two_views_of_one_buffer_have_independent_images():
    """One buffer read as [256, 512] (ld 512), as its left half [256, 256] (ld 512) and as [512, 256] (ld 256): three keys at
    one address, three images, all correct -- also after the buffer is rewritten."""
    buf = fresh(256, 512).to(DEV)
    B512 = fresh(256, 512, scale=512 ** -0.5).to(DEV)
    B256 = fresh(256, 256, scale=256 ** -0.5).to(DEV)
    views = [(buf, 256, 512, 512), (buf, 256, 256, 512), (buf, 512, 256, 256)]
    L = Launch(GEMM_NT, [(views[0], B512), (views[1], B256), (views[2], B256)])
    L.run()
    L.check("three views")
    assert all((buf.data_ptr(),) + v[1:] in ops._X3_BUFFERS for v in views), "one image per (address, rows, cols, ld)"
    buf.copy_(fresh(256, 512))
    L.run()
    L.check("three views, buffer rewritten")
    # and the full-width view alone after the half-width one was split last (another table, the same images)
    L2 = Launch(GEMM_NT, [(views[0], B512)] * 3)
    buf.copy_(fresh(256, 512))
    L2.run()
    L2.check("full view in a table of its own")
