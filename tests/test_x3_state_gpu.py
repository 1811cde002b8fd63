"""The bf16x3 split-image cache (ops.X3Cache: images, static / static_splits, fresh / epoch; ops._X3Plan, x3_presplit) through
ops.gemm_grouped(..., x3=<a cache of the test's own>), without a model.  An operand's [hi | lo] bf16 image is cached per
(address, rows, cols, ld) in the cache the launch is given, and lives as long as that cache; a weight's image is refreshed
only by refresh_static(), an activation's is skipped when an earlier launch of the same step through the same cache left it,
and that decision is frozen when the launch's plan is built.  A stale image gives finite, plausible numbers:
every result here is compared with the fp64 product of the fp32 operands AS THEY ARE IN MEMORY WHEN THE LAUNCH RUNS, at the
bf16x3 limit of tests/test_kernels_gpu.py::test_gemm_bf16x3_products (5e-5 of the result's scale); rewritten operands are
fresh draws, so a stale image is off by the scale itself.

Launch sizes: NT / NN three problems of 256 x 256 x 256 (as test_gemm_bf16x3_products pads its launches); TN 24 problems of
512 x 512 x 256 = 96 tiles of 256 x 256, the least a weight-gradient launch needs for the split path."""
import gc

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
    problem array is built once and replayed, like a launch table of the engine.  `cache`: the ops.X3Cache that owns the
    operands' split images."""

    def __init__(self, cache, variant, pairs, presplit=()):
        self.cache, self.variant, self.pairs, self.outs, probs = cache, variant, pairs, [], []
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
        ops.gemm_grouped(BPM_F32, self.variant, self.arr, x3=self.cache)
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


def plain_launch(cache, variant, shared=None, side="A"):
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
    return Launch(cache, variant, pairs)


@pytest.mark.parametrize("variant", [GEMM_NT, GEMM_NN, GEMM_TN], ids=NAMES.get)
def test_dynamic_operand_rewritten_in_place(variant):
    """The same problem array launched twice with both operands rewritten in place in between: the second result follows the
    new values (an activation buffer of the hot path: same address every step, new contents)."""
    L = plain_launch(ops.X3Cache(torch.device(DEV)), variant)
    L.run()
    L.check("first launch")
    for a, b in {(id(a), id(b)): (a, b) for a, b in L.pairs}.values():
        a.copy_(fresh(*a.shape))
        b.copy_(fresh(*b.shape, scale=256 ** -0.5))
    L.run()
    L.check("after the operands were rewritten in place")


@pytest.mark.parametrize("variant", [GEMM_NT, GEMM_NN], ids=NAMES.get)
def test_static_range_follows_refresh_and_drop(variant):
    """A weight buffer inside a static range of its store's cache (ParamStore.finalize_shadows): split when a plan first meets
    it, again only by refresh_static() (ParamStore.refresh_shadows) -- after which the result follows the new weights -- and,
    once the store's cache is gone (the store is gone), split on every launch of a new table through a cache without that
    range, like any other operand."""
    _, sb = operand_shapes(variant, 256, 256, 256)
    W = fresh(*sb, scale=256 ** -0.5).to(DEV)                # the B operand of the forward (NT) and data-gradient (NN) products
    lo = W.data_ptr()
    rng = (lo, lo + W.numel() * W.element_size())
    store = ops.X3Cache(W.device)                            # the store's cache: owns the range, the weight's image and its split
    store.add_static(*rng)
    cache = ops.X3Cache(W.device, weights=store)             # a trunk's: the activations' images
    L = plain_launch(cache, variant, shared=W, side="B")
    L.run()
    L.check("first launch over the static range")
    assert any(k[0] == lo for k in store.static_splits), "the weight buffer was taken as a static operand"
    assert any(k[0] == lo for k in store.images) and not any(k[0] == lo for k in cache.images), "its image is the store's"
    old = W.cpu().clone()
    W.copy_(fresh(*sb, scale=256 ** -0.5))
    L.run()                                                  # no refresh yet: the image is the old weights' (that is the
    stale = L.errors([(Launch._values(a), old) for a, _ in L.pairs])          # caching this file is about -- it is real)
    assert max(stale) <= X3_TOL, f"before refresh_static() the launch still reads the image of the old weights: {max(stale):.2e}"
    store.refresh_static()
    L.run()
    L.check("after the weights were rewritten and refresh_static()")
    torch.cuda.synchronize()
    del L, cache, store                                      # the store and what launched over it are gone
    gc.collect()
    cache = ops.X3Cache(W.device)                            # a new owner that has no such range
    assert not any(k[0] == lo for k in cache.static_splits) and rng not in cache.static
    L2 = plain_launch(cache, variant, shared=W, side="B")    # a new launch table over the same address
    L2.run()
    L2.check("first launch after the store's cache was dropped")
    W.copy_(fresh(*sb, scale=256 ** -0.5))
    L2.run()                                                 # no refresh: a dynamic operand is split by every launch
    L2.check("rewritten after the store's cache was dropped, no refresh")
    assert not any(k[0] == lo for k in cache.static_splits)


def _presplit_pair(cache, cache2=None):
    """Launch 1 (NT, a forward product) splits the activation X [256, 512]; launch 2 (TN, the weight gradient that reads X
    again as its B operand: the same (address, rows, cols, ld)) is tagged x3_presplit = {X}.
    Both go through `cache`, or launch 2 through `cache2`."""
    X = fresh(256, 512).to(DEV)
    Ws = [fresh(256, 512, scale=512 ** -0.5).to(DEV) for _ in range(3)]
    L1 = Launch(cache, GEMM_NT, [(X, w) for w in Ws])
    dY = [fresh(256, 512, scale=256 ** -0.5).to(DEV) for _ in range(2)]
    L2 = Launch(cache2 or cache, GEMM_TN, [(dY[i % 2], X) for i in range(24)], presplit=(X,))
    return X, L1, L2


def test_presplit_image_is_reused_within_a_step_and_renewed_in_the_next():
    cache = ops.X3Cache(torch.device(DEV))
    X, L1, L2 = _presplit_pair(cache)
    cache.new_step()
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
        cache.new_step()
        X.copy_(fresh(256, 512))
        L1.run()
        L2.run()
        L1.check(f"launch 1, step {step + 1}")
        L2.check(f"launch 2 (x3_presplit), step {step + 1}: X was rewritten")


def test_presplit_across_two_streams_ordered_by_an_event():
    """As the engine runs its weight gradients: launch 1 on the main stream, launch 2 on a side stream behind an event."""
    cache = ops.X3Cache(torch.device(DEV))
    X, L1, L2 = _presplit_pair(cache)
    main, side = torch.cuda.current_stream(), torch.cuda.Stream()

    def step():
        cache.new_step()
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
    """Images are keyed by raw address within their cache: an operand is freed and another tensor of the same shape
    allocated, launched through the SAME cache (a trunk's conv buffers, say).  When the allocator hands out the same address
    (it does for a same-size block), the result must use the new contents."""
    side = "A" if variant == GEMM_NT else "B"
    sa, sb = operand_shapes(variant, *((256, 256, 256) if variant == GEMM_NT else (512, 512, 256)))
    shape = sa if side == "A" else sb
    X1 = fresh(*shape).to(DEV)
    ptr = X1.data_ptr()
    cache = ops.X3Cache(torch.device(DEV))
    L = plain_launch(cache, variant, shared=X1, side=side)
    L.run()
    L.check("first tensor")
    torch.cuda.synchronize()
    del L, X1
    X2 = torch.empty(*shape, device=DEV)
    X2.copy_(fresh(*shape))
    same = X2.data_ptr() == ptr
    with capsys.disabled():
        print(f"\n[x3 address reuse, {NAMES[variant]}] the allocator returned {'the SAME address' if same else 'ANOTHER address'}")
    L = plain_launch(cache, variant, shared=X2, side=side)
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
    cache = ops.X3Cache(torch.device(DEV))
    L = Launch(cache, GEMM_NT, [(views[0], B512), (views[1], B256), (views[2], B256)])
    L.run()
    L.check("three views")
    assert all((buf.data_ptr(),) + v[1:] in cache.images for v in views), "one image per (address, rows, cols, ld)"
    buf.copy_(fresh(256, 512))
    L.run()
    L.check("three views, buffer rewritten")
    # and the full-width view alone after the half-width one was split last (another table, the same images)
    L2 = Launch(cache, GEMM_NT, [(views[0], B512)] * 3)
    buf.copy_(fresh(256, 512))
    L2.run()
    L2.check("full view in a table of its own")


def test_a_bool_is_no_cache():
    """There is no process-wide cache to fall back on: x3=True (the earlier form) is refused, as a tag on the table too."""
    L = plain_launch(True, GEMM_NT)
    with pytest.raises(TypeError):
        L.run()
    L.arr.x3 = True
    with pytest.raises(TypeError):
        ops.gemm_grouped(BPM_F32, GEMM_NT, L.arr)


def _image_bytes(cache):
    return sum(t.numel() * t.element_size() for t in cache.images.values())


def test_images_die_with_their_owner():
    """One NT launch of three 256 x 256 x 256 problems through a fresh cache: six images of rows x 2 ldp x 2 B = 256 KiB.  With
    the launch (its plan points into the cache) and the cache gone, their memory is free again -- the operands and outputs
    are kept alive here, so the images are all that can account for it."""
    cache = ops.X3Cache(torch.device(DEV))
    L = plain_launch(cache, GEMM_NT)
    L.run()
    L.check("the launch")
    torch.cuda.synchronize()
    m1, img = torch.cuda.memory_allocated(), _image_bytes(cache)
    assert len(cache.images) == 6 and img == 6 * 256 * 1024
    keep = (L.pairs, L.outs)                                 # noqa: F841 -- everything of the launch but its images
    del L, cache
    gc.collect()
    m2 = torch.cuda.memory_allocated()
    assert m2 <= m1 - img, f"allocated {m1} B with the cache, {m2} B without it: its {img} B of images are still held"


def test_two_caches_share_nothing():
    """Launch 1 splits X through cache a; X is rewritten; launch 2 (x3_presplit = {X}) runs in the same step through cache b:
    b has no record of a's split and no image of X, so it splits X itself.  Every image is on its operand's device."""
    a, b = ops.X3Cache(torch.device(DEV)), ops.X3Cache(torch.device(DEV))
    X, L1, L2 = _presplit_pair(a, b)
    L1.run()
    L1.check("launch 1 through cache a")
    X.copy_(fresh(256, 512))
    L2.run()
    L2.check("launch 2 (x3_presplit) through cache b, X rewritten after cache a's split")
    assert all(x.data_ptr() != y.data_ptr() for x in a.images.values() for y in b.images.values()), "an image in both caches"
    assert a.images and b.images and all(t.device == X.device for c in (a, b) for t in c.images.values())


def test_trunk_churn_is_bounded(monkeypatch):
    """The smallest model whose launches split (test_training_steps_gpu.SHAPES["x3"]), bf16x3, graphs off: one forward and
    backward at batch sizes 2, 3, 4 and the same cycle again.  A model keeps two trunks, so every step after the second batch
    size drops one -- with its cache.  The second cycle must leave as many images as the first (in the live trunks' caches and
    in the store's) and as much memory, to within less than one smallest image (256 KiB).
    Memory is what the program holds: the caching allocator's `requested_bytes`.  torch.cuda.memory_allocated() also counts
    the unused rest of a cached block handed out whole (up to 1 MiB a block, by which block happened to be free): measured
    here over four cycles, requested 1541872460 B after every cycle, allocated 1544166400 / 1547312128 / 1547312128 /
    1547312128 B -- the 3 MiB between the first two cycles is that slack, no tensor (the live storages sum to the requested
    figure); it is printed, not asserted."""
    from test_training_steps_gpu import NCLS, ORIG_A, ORIG_L, ORIG_V, SHAPES, build_model
    s = SHAPES["x3"]
    model = build_model("x3", "bf16x3").cuda().train()
    model.use_graphs = False
    split_ran, plan_run = set(), ops._X3Plan.run

    def counted_run(self, L, variant, seed, s_):
        assert self.ok
        split_ran.add(variant)
        return plan_run(self, L, variant, seed, s_)

    monkeypatch.setattr(ops._X3Plan, "run", counted_run)
    g = torch.Generator().manual_seed(5)
    data = {B: [torch.randn(B, T, D, generator=g).cuda() for T, D in ((s["L"], ORIG_L), (s["V"], ORIG_V), (s["A"], ORIG_A))] +
               [(torch.rand(B, NCLS, generator=g) > 0.5).float().cuda()] for B in (2, 3, 4)}
    seen = []
    for cycle in range(2):
        for B in (2, 3, 4):
            xl, img, aud, tgt = data[B]
            model.zero_grad(set_to_none=False)
            out = model(xl, None, None, img, aud)
            torch.nn.functional.binary_cross_entropy_with_logits(out, tgt).backward()
            assert torch.isfinite(out).all()
            del out
        torch.cuda.synchronize()
        gc.collect()
        assert sorted(model._trunks) == [3, 4] and all(t.x3.weights is model._store.x3_cache for t in model._trunks.values())
        seen.append((sum(len(t.x3.images) for t in model._trunks.values()), len(model._store.x3_cache.images),
                     torch.cuda.memory_stats()["requested_bytes.all.current"], torch.cuda.memory_allocated()))
    assert split_ran == {GEMM_NT, GEMM_NN, GEMM_TN}, f"split launches of all three operand arrangements must run: {split_ran}"
    (n1, w1, m1, a1), (n2, w2, m2, a2) = seen
    print(f"\n[x3 trunk churn] images {n1} -> {n2} (weights {w1} -> {w2}), held {m1} -> {m2} B (blocks: {a1} -> {a2} B)")
    assert n1 > 0 and w1 > 0
    assert (n2, w2) == (n1, w1), f"images after cycle 1: {n1} (+ {w1} of weights), after cycle 2: {n2} (+ {w2})"
    assert m2 - m1 < 256 * 1024, f"memory held grew by {m2 - m1} B over a cycle of dropped trunks"
