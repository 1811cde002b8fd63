"""Global-norm gradient clipping on the MI355X: the table-driven sum-of-squares reduction (bpm_grad_sumsq) against fp64,
its determinism and finalisation, the Adam entry that reads its gradient scale from the device
(bpm_adam_step_table_clip), and FusedAdam(max_grad_norm=...) / optim.grad_norm against torch.nn.utils.clip_grad_norm_.

Tolerance of every norm comparison: 2e-6 relative.  The reduction sums at most 16 squares per lane in one fp32 chain, an
8-level fp32 tree per block, and everything above in fp64: (1 + 16 + 8) * 2^-24 = 1.5e-6 on the sum of squares, half of
it under the root, plus the norm's rounding to fp32 (6e-8) -- 0.8e-6 in all."""
import copy
import math

import numpy as np
import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import ops  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.optim import FusedAdam, grad_norm  # noqa: E402
from test_model_gpu import args_for  # noqa: E402

DEV = "cuda"
REL = 2e-6
POISON = 1e30
LENGTHS = [1, 3, 4, 5, 1023, 1024, 1025, 4096 + 64, 3 * 4096 + 7]
BIG = 1_500_003                                            # one segment over 367 blocks


def lay_out(lengths, seed):
    """Segments cut from one randn buffer: every gap holds POISON, the start offsets walk through all four residues of
    (element offset mod 4) for every length, and each segment has a magnitude of its own in 1e-6 .. 1."""
    g = torch.Generator().manual_seed(seed)
    segs, cur = [], 0
    for k, n in enumerate(lengths):
        res = (k % len(LENGTHS) + k // len(LENGTHS)) % 4
        off = cur + 1
        while off % 4 != res:
            off += 1
        segs.append((off, n))
        cur = off + n
    buf = torch.full((cur + 8,), POISON)
    for off, n in segs:
        buf[off:off + n] = torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-6, 1, (1,), generator=g)))
    return buf.to(DEV), segs


class Reduction:
    """One table over `segs` of `buf`, with its workspace."""

    def __init__(self, buf, segs):
        assert buf.data_ptr() % 16 == 0
        self.buf = buf
        self.table = ops.sumsq_table([(buf.data_ptr() + 4 * off, n) for off, n in segs])
        self.ws = torch.full((ops.grad_sumsq_ws_bytes(self.table[2]) // 4,), float("nan"), device=DEV)

    def __call__(self, out=None, **kw):
        out = torch.zeros(2, device=DEV) if out is None else out
        ops.grad_sumsq(*self.table, self.ws, out, **kw)
        return out


@pytest.fixture(scope="module")
def laid():
    buf, segs = lay_out(LENGTHS * 4 + [BIG], seed=11)
    assert {off % 4 for off, n in segs if n == 1} == {0, 1, 2, 3}
    ref = [float(torch.linalg.vector_norm(buf[off:off + n].double())) for off, n in segs]
    return buf, segs, ref


def rel(a, b):
    return abs(a - b) / abs(b)


def test_reduction_matches_fp64(laid):
    """All segments in one table, and every segment as a table of its own (so that no segment hides behind a larger one),
    against torch.linalg.vector_norm of the same elements in fp64 to 2e-6 relative (module docstring).  A read outside a
    segment would meet 1e30."""
    buf, segs, ref = laid
    total = math.sqrt(sum(r * r for r in ref))
    got = Reduction(buf, segs)()
    torch.cuda.synchronize()
    print("whole table:", float(got[0]), total, rel(float(got[0]), total))
    assert rel(float(got[0]), total) <= REL and float(got[1]) == 1.0
    outs = torch.zeros(len(segs), 2, device=DEV)
    for i, s in enumerate(segs):
        Reduction(buf, [s])(outs[i])
    outs = outs.cpu()
    worst = max(rel(float(outs[i, 0]), ref[i]) for i in range(len(segs)))
    print("worst single segment:", worst)
    for i, (off, n) in enumerate(segs):
        assert rel(float(outs[i, 0]), ref[i]) <= REL, (off % 4, n, float(outs[i, 0]), ref[i])
    # the block count follows the start's offset inside its 16-byte line: 4096 elements at residue 1 take two blocks
    assert Reduction(buf, [(4, 4096)]).table[2] == 1 and Reduction(buf, [(5, 4096)]).table[2] == 2
    assert Reduction(buf, segs).table[2] >= BIG // 4096 + len(segs) - 1


def test_reduction_is_deterministic(laid):
    """Bit-equal output of two launches on the same data, and of a third after the same workspace has reduced other data
    in between: nothing is carried from one launch to the next."""
    buf, segs, _ = laid
    red = Reduction(buf, segs)
    c = 0.5 * float(red()[0])
    a = red(max_norm=c).clone()
    b = red(max_norm=c).clone()
    other, osegs = lay_out(LENGTHS + [70_001], seed=12)
    ored = Reduction(other, osegs)
    ored.ws = red.ws                                       # the same workspace (it is larger than this table needs)
    mid = ored(max_norm=c).clone()
    red.ws.fill_(float("inf"))
    third = red(max_norm=c).clone()
    assert torch.equal(a, b) and torch.equal(a, third) and not torch.equal(a, mid)
    assert 0.0 < float(a[1]) < 1.0


def test_finalisation(laid):
    buf, segs, ref = laid
    segs, ref = segs[:9], ref[:9]
    red = Reduction(buf, segs)
    sumsq = sum(r * r for r in ref)
    norm = float(red()[0])
    assert rel(norm, math.sqrt(sumsq)) <= REL
    # clipping: torch's formula in fp32, to 1 ulp
    below = 0.5 * norm
    out = red(max_norm=below).cpu().numpy()
    want = np.float32(below) / (np.float32(norm) + np.float32(1e-6))
    assert out[0] == np.float32(norm)
    assert abs(float(out[1]) - float(want)) <= float(np.spacing(want)), (out[1], want)
    assert 0.49 < out[1] < 0.51
    assert float(red(max_norm=2.0 * norm)[1]) == 1.0
    for only_norm in (0.0, -1.0, float("inf")):
        out = red(max_norm=only_norm)
        assert float(out[1]) == 1.0 and float(out[0]) == norm
    # grad_scale scales the norm (a power of two: exactly) and acts before the clip
    out = red(grad_scale=0.25, max_norm=below)
    assert float(out[0]) == 0.25 * norm and float(out[1]) == 1.0
    out = red(grad_scale=0.25, max_norm=0.25 * below)
    assert 0.49 < float(out[1]) < 0.51
    # extra_sumsq adds under the root
    extra = torch.tensor([3.0 * sumsq], device=DEV)
    assert rel(float(red(extra_sumsq=extra)[0]), 2.0 * math.sqrt(sumsq)) <= REL
    assert rel(float(red(grad_scale=0.5, extra_sumsq=extra)[0]), math.sqrt(sumsq)) <= REL
    # a non-finite norm propagates into the coefficient, as torch's clamp lets it
    nan = red(max_norm=1.0, extra_sumsq=torch.tensor([float("nan")], device=DEV))
    assert math.isnan(float(nan[0])) and math.isnan(float(nan[1]))


# ----------------------------------------------------------------------------------------------------------------------
def toy(hidden=24, layers=1, **kw):
    m = get_model(args_for("mmtrvat", hidden_sz=hidden, num_heads=4, layers=layers, orig_d_l=32, **kw))
    m.precision = "f32"
    return m


def toy_inputs():
    x = [torch.randn(2, 50, 32, device=DEV), torch.randn(2, 500, 35, device=DEV), torch.randn(2, 375, 74, device=DEV)]
    return x, (torch.randn(2, 6, device=DEV) > 0).float()


def backward(m, x, tgt):
    loss = torch.nn.functional.binary_cross_entropy_with_logits(m(x[0], None, None, x[1], x[2]), tgt)
    loss.backward()
    return loss


def composed_norm(m, st, grad_of=lambda n, p: p.grad):
    """The reference pieces under one root: fp64 sum of squares of the trunk gradients, plus the squares of
    torch._foreach_norm of the tail gradients."""
    trunk = [grad_of(n, p) for n, p in m.named_parameters() if n in st.params and grad_of(n, p) is not None]
    tail = [p.grad for n, p in m.named_parameters() if n not in st.params and p.grad is not None]
    s = torch.stack([g.double().square().sum() for g in trunk]).sum()
    if tail:
        s = s + torch.stack(torch._foreach_norm(tail)).double().square().sum()
    return math.sqrt(float(s))


def test_adam_with_a_device_scale():
    """bpm_adam_step_table_clip on the flat buffers of a store with column padding (hidden 40: leading dimension 64) and
    parameter padding: *scale_dev == 1 is bit-equal to bpm_adam_step_table (master, both moments, shadows); with
    scale 0.37 and grad_scale 0.5 the master follows torch.optim.Adam fed 0.185 * the gradients (2e-6 max-abs, the limit
    of test_fused_adam_kernel_exact); the plain shadows it wrote are bit-equal to a forced refresh."""
    torch.manual_seed(3)
    m = toy(hidden=40, num_vectors_l=48, num_vectors_a=48, num_vectors_v=48).cuda()
    st = m._ensure_store()
    assert st.total > sum(p.numel() for p in st.params.values())          # parameter padding exists
    st.refresh_shadows(force=True)
    g = torch.Generator().manual_seed(4)
    n = st.total
    grads = [(torch.randn(n, generator=g) * (10.0 ** float(torch.randint(-6, 1, (1,), generator=g)))).to(DEV) for _ in range(3)]
    master0, shadow0 = st.master.clone(), st.shadow_flat.clone()
    m0 = (torch.randn(n, generator=g) * 1e-2).to(DEV)
    v0 = (torch.rand(n, generator=g) * 1e-4).to(DEV)
    hp = dict(lr=3e-3, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.01)

    def run(scale_dev):
        st.master.copy_(master0)
        st.shadow_flat.copy_(shadow0)
        st.gflat.copy_(grads[0])
        ma, va = m0.clone(), v0.clone()
        st.adam_step(ma, va, step=2, grad_scale=0.5, zero_grad=False, scale_dev=scale_dev, **hp)
        return st.master.clone(), ma, va, st.shadow_flat.clone()

    plain = run(None)
    one = run(torch.ones(1, device=DEV))
    for a, b, what in zip(plain, one, ("master", "exp_avg", "exp_avg_sq", "shadows")):
        assert torch.equal(a, b), what
    assert not torch.equal(plain[0], master0)

    ref = master0.clone().requires_grad_(True)
    opt = torch.optim.Adam([ref], lr=3e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01)
    st.master.copy_(master0)
    ma, va = torch.zeros(n, device=DEV), torch.zeros(n, device=DEV)
    scale = torch.tensor([0.37], device=DEV)
    for it, gr in enumerate(grads, 1):
        ref.grad = gr * 0.185
        opt.step()
        st.gflat.copy_(gr)
        st.adam_step(ma, va, step=it, grad_scale=0.5, zero_grad=True, scale_dev=scale, **hp)
        assert float(st.gflat.abs().max()) == 0.0
        d = float((st.master - ref.detach()).abs().max())
        print("step", it, "max-abs", d)
        assert d <= 2e-6, (it, d)
    assert st._dirty_rest and not st._dirty
    st.refresh_shadows()                                    # the rest pass only
    got = st.shadow_flat.clone()
    st.refresh_shadows(force=True)
    assert torch.equal(got, st.shadow_flat)


LR_CLIP = 1e-4


def test_fused_adam_clips_like_torch():
    """FusedAdam(max_grad_norm=c) against torch.optim.Adam behind torch.nn.utils.clip_grad_norm_(.., c), three steps with
    a clip that bites at every one (c = half of the first norm); last_grad_norm against the norm composed from reference
    pieces on the same gradients.  Limits of test_fused_adam_matches_torch_adam: losses 1e-5, parameters 3e-3.

    Learning rate 1e-4, not that test's 1e-2: Adam moves every element by ~lr per step whatever the gradient's size, and
    this model's gradient norm falls fast under it -- measured on the torch copy, 2.98 -> 0.85 after one step at 1e-2 and
    2.98 -> 1.82 -> 1.08 at 1e-3 -- so at either the norm is under c = 1.49 before the third step and the clip would not
    bite at every step.  The fall per step scales with lr (71 % at 1e-2, 39 % at 1e-3); at 1e-4 it is a few per cent.
    That test's parameter limit is a tenth of the 3 * lr an element can travel; the same tenth of the smaller travel,
    3e-5, is asserted here as well."""
    torch.manual_seed(7)
    m1 = toy(layers=2)
    m2 = copy.deepcopy(m1)
    m1, m2 = m1.cuda().train(), m2.cuda().train()
    x, tgt = toy_inputs()
    backward(m1, x, tgt)
    c = 0.5 * float(torch.nn.utils.clip_grad_norm_(m1.parameters(), float("inf")))
    o1 = torch.optim.Adam(m1.parameters(), lr=LR_CLIP, weight_decay=0.0)
    o2 = FusedAdam(m2, lr=LR_CLIP, max_grad_norm=c)
    assert o2.last_grad_norm is None
    for it in range(3):
        o1.zero_grad()
        l1 = float(backward(m1, x, tgt).detach())
        n1 = float(torch.nn.utils.clip_grad_norm_(m1.parameters(), c))
        print("step", it, "torch norm", n1, "c", c)
        assert n1 > c, (it, n1, c)
        o1.step()
        o2.zero_grad()
        l2 = float(backward(m2, x, tgt).detach())
        want = composed_norm(m2, m2._store)
        o2.step()
        got = o2.last_grad_norm
        assert got.is_cuda and got.dim() == 0 and got.dtype == torch.float32
        print("step", it, "norm", float(got), want, n1, "losses", l1, l2)
        assert rel(float(got), want) <= REL, (it, float(got), want)
        assert abs(l1 - l2) <= 1e-5 * max(1.0, abs(l1)), (it, l1, l2)
    worst = 0.0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        worst = max(worst, float((p1.detach() - p2.detach()).abs().max()))
    print("worst parameter difference", worst)
    assert worst <= 3e-3 and worst <= 0.1 * 3 * LR_CLIP, worst


def given_grads(m, seed, mult=1.0):
    """The same gradients for every copy of a model: the flat buffer and the tail's .grad from one generator."""
    st = m._ensure_store()
    g = torch.Generator().manual_seed(seed)
    st.gflat.copy_((torch.randn(st.total, generator=g) * mult).to(DEV))
    for n, p in m.named_parameters():
        if n not in st.params:
            p.grad = (torch.randn(p.shape, generator=g) * mult).to(DEV)
    return st


def test_grad_scale_acts_before_the_clip():
    """step(grad_scale=0.25) on given gradients == a step on the gradients multiplied by 0.25 beforehand (what GradSync's
    1 / world after a sum all-reduce means), and last_grad_norm is 0.25 x the norm of the unscaled gradients."""
    torch.manual_seed(9)
    m1 = toy()
    m2 = copy.deepcopy(m1)
    m1, m2 = m1.cuda(), m2.cuda()
    st1 = given_grads(m1, 21)
    unscaled = composed_norm(m1, st1, grad_of=lambda n, p: st1.g(n))
    c = 0.5 * 0.25 * unscaled
    o1 = FusedAdam(m1, lr=1e-2, max_grad_norm=c)
    o1.step(grad_scale=0.25)
    given_grads(m2, 21, mult=0.25)
    o2 = FusedAdam(m2, lr=1e-2, max_grad_norm=c)
    o2.step()
    assert rel(float(o1.last_grad_norm), 0.25 * unscaled) <= REL
    assert rel(float(o2.last_grad_norm), 0.25 * unscaled) <= REL
    worst = 0.0
    for (k, p1), (_, p2) in zip(m1.named_parameters(), m2.named_parameters()):
        worst = max(worst, float((p1.detach() - p2.detach()).abs().max()))
    print("worst parameter difference", worst)
    assert worst <= 2e-6, worst
    # a pending scale left by GradSync.finish() is consumed the same way
    st1 = given_grads(m1, 22)
    unscaled = composed_norm(m1, st1, grad_of=lambda n, p: st1.g(n))
    o1.pending_grad_scale = 0.25
    o1.step()
    assert o1.pending_grad_scale is None and rel(float(o1.last_grad_norm), 0.25 * unscaled) <= REL


def test_norm_covers_the_trainable_parameters_only():
    """A frozen trunk parameter's slice of the flat gradient buffer is still filled by the backward launches, and must
    not count; neither does a frozen tail parameter."""
    torch.manual_seed(13)
    m = toy().cuda().train()
    frozen = "trans_l_with_a.layers.0.fc1.weight"
    dict(m.named_parameters())[frozen].requires_grad_(False)
    m.out_layer.bias.requires_grad_(False)
    x, tgt = toy_inputs()
    backward(m, x, tgt)
    st = m._store
    assert frozen in st.params and "out_layer.bias" not in st.params
    assert dict(m.named_parameters())[frozen].grad is None and m.out_layer.bias.grad is None
    sl = st.g(frozen)
    assert float(sl.abs().max()) > 0.0
    want = composed_norm(m, st)
    got = float(grad_norm(m))
    with_frozen = math.sqrt(want * want + float(sl.double().square().sum()))
    print("norm", got, "reference", want, "with the frozen slice", with_frozen)
    assert rel(got, want) <= REL
    assert rel(got, with_frozen) > 10 * REL                 # an order above what the tolerance could hide
    assert rel(float(grad_norm(m, grad_scale=0.5)), 0.5 * want) <= REL
    # the optimizer sees the same set
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=1e6)
    before = st.gflat.clone()
    opt.step()
    assert rel(float(opt.last_grad_norm), want) <= REL and torch.equal(before, st.gflat)


def test_default_path_is_untouched():
    """Without max_grad_norm the step launches what it always launched: no reduction, no buffers, no norm.  The value
    travels with the optimizer's state_dict; a checkpoint without it keeps the constructor's."""
    torch.manual_seed(15)
    m = toy().cuda().train()
    with pytest.raises(RuntimeError, match="no gradients yet"):
        grad_norm(m)
    assert m._ensure_store()._norm_table is None
    x, tgt = toy_inputs()
    opt = FusedAdam(m, lr=1e-3)
    opt.zero_grad()
    backward(m, x, tgt)
    opt.step()
    st = m._store
    assert opt.last_grad_norm is None and st._norm_table is None
    assert not hasattr(st, "_norm_ws") and not hasattr(st, "_norm_out")
    sd = opt.state_dict()
    assert sd["param_groups"][0]["max_grad_norm"] is None
    clipped = FusedAdam(m, lr=1e-3, max_grad_norm=0.8)
    sd8 = clipped.state_dict()
    assert sd8["param_groups"][0]["max_grad_norm"] == 0.8
    opt.load_state_dict(sd8)
    assert opt.param_groups[0]["max_grad_norm"] == 0.8
    del sd["param_groups"][0]["max_grad_norm"]               # a checkpoint written before the key existed
    clipped.load_state_dict(sd)
    assert clipped.param_groups[0]["max_grad_norm"] == 0.8
    backward(m, x, tgt)
    clipped.step()
    assert float(clipped.last_grad_norm) > 0.0 and st._norm_table is not None
    norm_buffers = (st._norm_ws.data_ptr(), st._norm_out.data_ptr())
    clipped.step()
    assert norm_buffers == (st._norm_ws.data_ptr(), st._norm_out.data_ptr())      # allocated once
