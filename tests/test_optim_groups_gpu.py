"""FusedAdam's parameter groups on the MI355X: bpm_adam_step_groups against the recorded bits of the one-group table step
(bpm_adam_step_table / _clip are now entries into the same kernel) and against torch.optim.Adam with the same groups
(L2 and decoupled decay, parameters in no group, a step left out for a non-finite norm, a group added later), and the
Python surface end to end.

Kernel-level comparisons run on GIVEN gradients (one magnitude in 1e-6 .. 1 per parameter) and hold the project's kernel
limit, max-abs 2e-6 against torch (test_fused_adam_kernel_exact): an fp32 restatement of both updates stays within 2.4e-7
of torch.optim.Adam at learning rates <= 3e-3 over four steps, one of them left out."""
import copy
import ctypes as C
import hashlib
import json
import math
import os

import pytest
import torch

pytestmark = pytest.mark.gpu

from bpmult_amd import _lib, ops  # noqa: E402
from bpmult_amd.models import get_model  # noqa: E402
from bpmult_amd.optim import FusedAdam, decay_groups  # noqa: E402
from test_model_gpu import args_for  # noqa: E402

DEV = "cuda"
LIMIT = 2e-6
FC1 = "trans_l_with_a.layers.0.fc1.weight"
FC2 = "trans_l_with_a.layers.0.fc2.weight"


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


def flat_grads(st, seed):
    """A flat gradient buffer from one generator: every parameter at a magnitude of its own in 1e-6 .. 1, zero padding."""
    g = torch.Generator().manual_seed(seed)
    flat = torch.zeros(st.total)
    for n in st.names:
        k = st.params[n].numel()
        flat[st.off[n]: st.off[n] + k] = torch.randn(k, generator=g) * (10.0 ** float(torch.randint(-6, 1, (1,), generator=g)))
    return flat.to(DEV), g


def given_grads(m, seed):
    """The same gradients for every copy of a model: the flat buffer and the tail's .grad from one generator."""
    st = m._ensure_store()
    flat, g = flat_grads(st, seed)
    st.gflat.copy_(flat)
    for n, p in m.named_parameters():
        if n not in st.params:
            p.grad = (torch.randn(p.shape, generator=g) * (10.0 ** float(torch.randint(-6, 1, (1,), generator=g)))).to(DEV)
    return st


def clones(m, names=None):
    """Free-standing copies of the model's parameters for a torch.optim.Adam reference."""
    return {n: p.detach().clone().requires_grad_(True) for n, p in m.named_parameters() if names is None or n in names}


def copy_grads(m, ref):
    st = m._store
    named = dict(m.named_parameters())
    for n, r in ref.items():
        r.grad = (st.g(n) if n in st.params else named[n].grad).detach().clone()


def worst(m, ref):
    named = dict(m.named_parameters())
    d = torch.stack([(named[n].detach() - r.detach()).abs().max() for n, r in ref.items()])
    i = int(d.argmax())
    return float(d[i]), list(ref)[i]


def shadow_of(st, name):
    rows, cols, dst_ld, off = st._adam_plain[name]
    return st.shadow_flat[off: off + rows * dst_ld]


@pytest.fixture(scope="module")
def padded():
    """Hidden 40: column padding (leading dimension 64) and parameter padding; start values shared by the kernel tests."""
    torch.manual_seed(3)
    m = toy(hidden=40, num_vectors_l=48, num_vectors_a=48, num_vectors_v=48).cuda()
    st = m._ensure_store()
    assert st.total > sum(p.numel() for p in st.params.values())
    st.refresh_shadows(force=True)
    grads = [flat_grads(st, 40 + i)[0] for i in range(3)]
    return m, st, st.master.clone(), st.shadow_flat.clone(), grads


def sha256(t):
    return hashlib.sha256(t.detach().cpu().contiguous().numpy().tobytes()).hexdigest()


def test_one_group_is_the_existing_step(padded):
    """Every segment in group 0 with L2 decay, through ParamStore.adam_step_groups and through ParamStore.adam_step, with
    and without scale_dev: master, both moments and the shadows carry the SHA-256 digests that the separate one-group
    kernel of bpm_adam_step_table / _clip left for the same start values on the commit before it was folded into the
    grouped kernel (tests/golden/adam_one_group_digests.json; there the two kernels gave equal bits).  The flat
    bpm_adam_step is no stand-in for that record: its results were not bit-equal to the table kernel's on that commit.
    Independently of the record, the plain shadows are bit-equal to a forced refresh_shadows of the stepped masters and
    every other shadow element is untouched.  With the step count on the device the bias corrections are taken there
    (integer power by squaring instead of the host's pow): the kernel limit holds, and the counter advances."""
    m, st, master0, shadow0, grads = padded
    n = st.total
    g = torch.Generator().manual_seed(4)
    m0 = (torch.randn(n, generator=g) * 1e-2).to(DEV)
    v0 = (torch.rand(n, generator=g) * 1e-4).to(DEV)
    hp = dict(lr=3e-3, beta1=0.9, beta2=0.98, eps=1e-8, weight_decay=0.01)
    one = [dict(lr=3e-3, betas=(0.9, 0.98), eps=1e-8, weight_decay=0.01, step=2)]
    everyone = {k: 0 for k in st.names}
    plain = torch.zeros(st.shadow_flat.numel(), dtype=torch.bool, device=DEV)
    for rows, cols, dst_ld, off in st._adam_plain.values():
        plain[off: off + rows * dst_ld] = True
    assert bool(plain.any()) and not bool(plain.all())

    def run(grouped, scale_dev, steps_dev=None):
        st.master.copy_(master0)
        st.shadow_flat.copy_(shadow0)
        st.gflat.copy_(grads[0])
        ma, va = m0.clone(), v0.clone()
        if grouped:
            st.adam_step_groups(ma, va, st.adam_group_table(everyone), ops.adam_groups(one), 0.5, False, scale_dev=scale_dev, steps_dev=steps_dev)
        else:
            st.adam_step(ma, va, step=2, grad_scale=0.5, zero_grad=False, scale_dev=scale_dev, **hp)
        return st.master.clone(), ma, va, st.shadow_flat.clone()

    assert st.adam_group_table(everyone)[1:] == st._adam_table[1:]
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "adam_one_group_digests.json")) as f:
        want = json.load(f)
    names = ("master", "exp_avg", "exp_avg_sq", "shadows")
    cases = {"no_scale_dev": None, "scale_dev_0.37": torch.tensor([0.37], device=DEV)}
    results = {(key, grouped): run(grouped, scale) for key, scale in cases.items() for grouped in (False, True)}
    got = {"start_values": sha256(torch.cat([master0, shadow0.float(), grads[0], m0, v0]))}
    for (key, grouped), res in results.items():
        got[key + (" adam_step_groups" if grouped else " adam_step")] = dict(zip(names, map(sha256, res)))
    print(json.dumps(got))
    assert got["start_values"] == want["start_values"], "not the start values of the record: the digests cannot match"
    for (key, grouped), res in results.items():
        assert got[key + (" adam_step_groups" if grouped else " adam_step")] == want[key], (key, grouped)
        st.master.copy_(res[0])
        st.refresh_shadows(force=True)
        assert torch.equal(st.shadow_flat[plain], res[3][plain]), ("shadows", key, grouped)
        assert torch.equal(res[3][~plain], shadow0[~plain]), ("the other shadows", key, grouped)
        assert not torch.equal(res[0], master0) and not torch.equal(res[3][plain], shadow0[plain])
    steps = torch.tensor([1, 7], device=DEV, dtype=torch.int32)
    host, dev = run(False, None), run(True, None, steps_dev=steps)
    for a, b, what in zip(host[:3], dev[:3], ("master", "exp_avg", "exp_avg_sq")):
        d = float((a - b).abs().max())
        print("device step count,", what, "max-abs", d)
        assert d <= LIMIT, what
    assert steps.tolist() == [2, 7]
    st.master.copy_(master0)
    st.refresh_shadows(force=True)


def test_table_entries_ignore_the_group_word(padded):
    """bpm_adam_step_table on the store's table and on a copy whose segments carry 7 and -1 in their `group` words (a
    caller's table from before the word had a meaning may hold anything there): master, moments and shadows bit-equal."""
    m, st, master0, shadow0, grads = padded
    tab, nseg, nblk = st._adam_table
    words = C.sizeof(_lib.AdamSeg) // 4
    host = tab.cpu().view(torch.int32).view(nseg, words).clone()
    assert _lib.AdamSeg.group.offset == 4 * (words - 1) and nseg >= 2 and int(host[:, -1].abs().max()) == 0
    host[0::2, -1], host[1::2, -1] = 7, -1
    scribbled = host.view(-1).view(torch.uint8).to(DEV)
    g = torch.Generator().manual_seed(5)
    m0 = (torch.randn(st.total, generator=g) * 1e-2).to(DEV)
    v0 = (torch.rand(st.total, generator=g) * 1e-4).to(DEV)

    def run(table):
        st.master.copy_(master0)
        st.shadow_flat.copy_(shadow0)
        st.gflat.copy_(grads[1])
        ma, va = m0.clone(), v0.clone()
        _lib.check(_lib.lib().bpm_adam_step_table(st.dtype, table.data_ptr(), nseg, nblk, st.master.data_ptr(), st.gflat.data_ptr(),
                                                  ma.data_ptr(), va.data_ptr(), 3e-3, 0.9, 0.98, 1e-8, 0.01, 3, 0.5, 0,
                                                  torch.cuda.current_stream().cuda_stream), "bpm_adam_step_table")
        return st.master.clone(), ma, va, st.shadow_flat.clone()

    want, got = run(tab), run(scribbled)
    for a, b, what in zip(want, got, ("master", "exp_avg", "exp_avg_sq", "shadows")):
        assert torch.equal(a, b), what
    assert not torch.equal(want[0], master0) and not torch.equal(want[3], shadow0)
    st.master.copy_(master0)
    st.refresh_shadows(force=True)


def test_groups_against_torch(padded):
    """Three groups (L2, decoupled with betas of its own, the vectors without decay) and two parameters in none, three
    steps with one group's lr changed before the third, against torch.optim.Adam over clones with the same groups."""
    m, st, master0, shadow0, grads = padded
    st.master.copy_(master0)
    st.refresh_shadows(force=True)
    ln = next(k for k in st.names if "layer_norm" in k and k.endswith("weight"))
    out = (FC1, ln)
    assert FC1 in st._adam_plain and ln not in st._adam_plain
    group_of = {k: (2 if st.params[k].ndim <= 1 else 0 if k.startswith("trans_l") else 1) for k in st.names if k not in out}
    hyper = [dict(lr=3e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.01, decoupled_weight_decay=False),
             dict(lr=1e-3, betas=(0.8, 0.999), eps=1e-8, weight_decay=0.1, decoupled_weight_decay=True),
             dict(lr=1e-4, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, decoupled_weight_decay=False)]
    ref = {k: st.params[k].detach().clone().requires_grad_(True) for k in group_of}
    opt = torch.optim.Adam([dict(h, params=[ref[k] for k in group_of if group_of[k] == i]) for i, h in enumerate(hyper)])
    assert all(g["params"] for g in opt.param_groups)
    ma, va = torch.zeros(st.total, device=DEV), torch.zeros(st.total, device=DEV)
    named = dict(m.named_parameters())
    table = st.adam_group_table(group_of)
    for it, gr in enumerate(grads, 1):
        if it == 3:
            hyper[1]["lr"] = opt.param_groups[1]["lr"] = 4e-4
        st.gflat.copy_(gr)
        for k, r in ref.items():
            r.grad = st.g(k).clone()
        opt.step()
        st.adam_step_groups(ma, va, table, ops.adam_groups([dict(h, step=it) for h in hyper]), 1.0, it == 3)
        d = torch.stack([(named[k].detach() - r.detach()).abs().max() for k, r in ref.items()])
        i = int(d.argmax())
        print("step", it, "worst stepped parameter", float(d[i]), list(ref)[i], "group", group_of[list(ref)[i]])
        assert float(d[i]) <= LIMIT, (it, float(d[i]), list(ref)[i])
        if it < 3:
            assert torch.equal(st.gflat, gr)                                  # zero_grad=False: nothing written
        else:
            assert float(st.gflat.abs().max()) == 0.0                         # ... and with it, the unstepped slices too
            for k in out:
                assert float(gr[st.off[k]: st.off[k] + st.params[k].numel()].abs().max()) > 0.0
    assert not torch.equal(st.master, master0)
    for k in out:                                                             # not stepped: bits kept, moments never written
        a, b = st.off[k], st.off[k] + (st.params[k].numel() + 63) // 64 * 64
        assert torch.equal(st.master[a:b], master0[a:b]), k
        assert float(ma[a:b].abs().max()) == 0.0 and float(va[a:b].abs().max()) == 0.0, k
    rows, cols, dst_ld, off = st._adam_plain[FC1]
    assert torch.equal(shadow_of(st, FC1), shadow0[off: off + rows * dst_ld])
    off2 = st._adam_plain[FC2][3]
    assert not torch.equal(shadow_of(st, FC2), shadow0[off2: off2 + shadow_of(st, FC2).numel()])
    assert st._dirty_rest and not st._dirty
    st.refresh_shadows()                                                      # the rest pass only
    got, gotf = st.shadow_flat.clone(), st.fold_flat.clone()
    st.refresh_shadows(force=True)
    assert torch.equal(got, st.shadow_flat) and torch.equal(gotf, st.fold_flat)
    st.master.copy_(master0)
    st.refresh_shadows(force=True)


def test_frozen_stays_frozen():
    """requires_grad_(False) on a trunk weight and on a tail bias before the default construction: a real forward,
    backward and step move neither (the backward launches still fill the trunk one's gradient slice, and there is weight
    decay), and leave the trunk one's shadow and moments alone; an unfrozen neighbour moves."""
    torch.manual_seed(13)
    m = toy().cuda().train()
    named = dict(m.named_parameters())
    named[FC1].requires_grad_(False)
    m.out_layer.bias.requires_grad_(False)
    opt = FusedAdam(m, lr=1e-2, weight_decay=0.01)
    x, tgt = toy_inputs()
    backward(m, x, tgt)
    st = m._store
    assert FC1 in st.params and "out_layer.bias" not in st.params and float(st.g(FC1).abs().max()) > 0.0
    before = {k: named[k].detach().clone() for k in (FC1, FC2, "out_layer.bias", "out_layer.weight")}
    shadow = shadow_of(st, FC1).clone()
    opt.step()
    assert torch.equal(named[FC1].detach(), before[FC1])
    assert torch.equal(m.out_layer.bias.detach(), before["out_layer.bias"])
    assert torch.equal(shadow_of(st, FC1), shadow)
    a, b = st.off[FC1], st.off[FC1] + named[FC1].numel()
    assert float(opt._m[a:b].abs().max()) == 0.0 and float(opt._v[a:b].abs().max()) == 0.0
    assert not torch.equal(named[FC2].detach(), before[FC2]) and float(opt._m[st.off[FC2]: st.off[FC2] + 8].abs().max()) > 0.0
    assert not torch.equal(m.out_layer.weight.detach(), before["out_layer.weight"])
    assert len(opt.param_groups) == 1 and opt.state_dict()["step"] == 1


def full_state(m, opt):
    st = m._store
    out = [st.master.clone(), opt._m.clone(), opt._v.clone(), st.shadow_flat.clone()]
    for tg in opt._tail_opt.param_groups:
        for p in tg["params"]:
            s = opt._tail_opt.state[p]
            out += [p.detach().clone(), s["exp_avg"].clone(), s["exp_avg_sq"].clone(), s["step"].clone()]
    return out


@pytest.mark.parametrize("clip", [None, 1.0])
@pytest.mark.parametrize("poison", ["inf in the flat buffer", "nan in a tail gradient"])
def test_skip(poison, clip):
    """Step 1 finite, step 2 poisoned, step 3 finite: after step 2 everything is what step 1 left and the skip is counted;
    the end state is torch.optim.Adam's after the gradients of steps 1 and 3 only (so the bias corrections of step 3 are
    those of an optimizer's second step)."""
    torch.manual_seed(17)
    m = toy().cuda()
    st = m._ensure_store()
    st.refresh_shadows(force=True)
    ref = clones(m)
    topt = torch.optim.Adam(list(ref.values()), lr=3e-3, weight_decay=0.01)
    opt = FusedAdam(m, lr=3e-3, weight_decay=0.01, skip_nonfinite=True, fused_zero_grad=True, max_grad_norm=clip)
    assert int(opt.skipped_steps) == 0 and opt.skipped_steps.is_cuda and opt.skipped_steps.dim() == 0
    assert not opt.skipped_steps.dtype.is_floating_point

    def good(seed):
        given_grads(m, seed)
        copy_grads(m, ref)
        if clip is not None:
            n = float(torch.nn.utils.clip_grad_norm_(list(ref.values()), clip))
            assert n > clip
        topt.step()
        opt.step()
        assert math.isfinite(float(opt.last_grad_norm)) and float(st.gflat.abs().max()) == 0.0

    good(31)
    after1 = full_state(m, opt)
    given_grads(m, 32)
    if poison.startswith("inf"):
        st.g(FC1).view(-1)[5] = float("inf")
    else:
        m.out_layer.weight.grad.view(-1)[3] = float("nan")
    opt.step()
    assert not math.isfinite(float(opt.last_grad_norm))
    assert int(opt.skipped_steps) == 1
    assert float(st.gflat.abs().max()) == 0.0                                 # cleared all the same (the inf included)
    for i, (a, b) in enumerate(zip(after1, full_state(m, opt))):
        assert torch.equal(a, b), i
    good(33)
    w, name = worst(m, ref)
    print(poison, "clip", clip, "worst parameter", w, name)
    assert w <= LIMIT, (w, name)
    sd = opt.state_dict()
    assert sd["step"] == 2 and sd["group_steps"] == [2] and sd["skipped"] == 1 and sd["step_calls"] == 3 and opt.step_count == 3
    st.refresh_shadows()
    got = st.shadow_flat.clone()
    st.refresh_shadows(force=True)
    assert torch.equal(got, st.shadow_flat)


def test_step_never_waits_for_the_device():
    """After a warm-up step, a step with groups, clipping and skip_nonfinite under torch's sync debug mode "error": any
    host wait for the device inside step() raises."""
    torch.manual_seed(19)
    m = toy().cuda()
    opt = FusedAdam(m, lr=1e-3, skip_nonfinite=True, fused_zero_grad=True, max_grad_norm=1.0,
                    param_groups=decay_groups(m, 0.01, decoupled_weight_decay=True))
    given_grads(m, 51)
    opt.step()
    given_grads(m, 52)
    torch.cuda.synchronize()
    torch.cuda.set_sync_debug_mode("error")
    try:
        opt.step()
    finally:
        torch.cuda.set_sync_debug_mode("default")
    assert int(opt.skipped_steps) == 0 and opt.state_dict()["group_steps"] == [2, 2]


def named_groups(m, groups):
    named = {id(p): n for n, p in m.named_parameters()}
    return [[named[id(p)] for p in g["params"]] for g in groups]


def test_param_groups_end_to_end():
    """FusedAdam(param_groups=decay_groups + a third group holding out_layer.* at its own lr) against torch.optim.Adam
    with the same groups on a deep copy: three real training steps, a LambdaLR with one lambda per group between them.
    Limits of test_fused_adam_matches_torch_adam: losses 1e-5 relative; each parameter within a tenth of the 3 * lr its
    group can travel, and within 3e-3."""
    torch.manual_seed(7)
    m1 = toy(layers=2)
    m2 = copy.deepcopy(m1)
    m1, m2 = m1.cuda().train(), m2.cuda().train()
    x, tgt = toy_inputs()
    lrs = [1e-2, 5e-3, 2e-3]

    def groups_for(m):
        head = list(m.out_layer.parameters())
        gs = decay_groups(m, 0.01, decoupled_weight_decay=True)
        for g, lr in zip(gs, lrs):
            g["params"] = [p for p in g["params"] if all(p is not h for h in head)]
            g["lr"] = lr
        return gs + [dict(params=head, lr=lrs[2], weight_decay=0.0)]

    o1 = torch.optim.Adam(groups_for(m1), lr=1e-3)
    o2 = FusedAdam(m2, lr=1e-3, param_groups=groups_for(m2))
    assert named_groups(m1, o1.param_groups) == named_groups(m2, o2.param_groups) and len(o2.param_groups) == 3
    assert [g["decoupled_weight_decay"] for g in o2.param_groups] == [True, True, False]
    lam = [lambda e: 0.5 ** e, lambda e: 1.0, lambda e: 0.9 ** e]
    s1, s2 = torch.optim.lr_scheduler.LambdaLR(o1, lam), torch.optim.lr_scheduler.LambdaLR(o2, lam)
    for it in range(3):
        losses = []
        for m, o, s in ((m1, o1, s1), (m2, o2, s2)):
            o.zero_grad()
            losses.append(float(backward(m, x, tgt).detach()))
            o.step()
            s.step()
        print("step", it, "losses", losses)
        assert abs(losses[0] - losses[1]) <= 1e-5 * max(1.0, abs(losses[0])), (it, losses)
    assert [g["lr"] for g in o1.param_groups] == [g["lr"] for g in o2.param_groups]
    assert abs(o2.param_groups[0]["lr"] - lrs[0] / 8) < 1e-12
    group_lr = {n: lr for names, lr in zip(named_groups(m2, o2.param_groups), lrs) for n in names}
    p1 = dict(m1.named_parameters())
    for lr in lrs:
        w = max(float((p1[n].detach() - p.detach()).abs().max()) for n, p in m2.named_parameters() if group_lr[n] == lr)
        print("group lr", lr, "worst parameter difference", w, "limit", min(3e-3, 0.1 * 3 * lr))
        assert w <= 3e-3 and w <= 0.1 * 3 * lr, (lr, w)
    assert o2.state_dict()["group_steps"] == [3, 3, 3]


def test_add_param_group():
    """Two steps with a matrix frozen, then requires_grad_(True) and add_param_group: two more steps against torch doing
    the same.  Within the kernel limit only if the new group's bias corrections start from its own step 1."""
    torch.manual_seed(23)
    m = toy().cuda()
    st = m._ensure_store()
    named = dict(m.named_parameters())
    named[FC1].requires_grad_(False)
    ref = clones(m)
    topt = torch.optim.Adam([r for n, r in ref.items() if n != FC1], lr=3e-3, weight_decay=0.01)
    opt = FusedAdam(m, lr=3e-3, weight_decay=0.01)
    fc1 = named[FC1].detach().clone()
    for it in range(4):
        if it == 2:
            assert torch.equal(named[FC1].detach(), fc1)
            named[FC1].requires_grad_(True)
            opt.add_param_group({"params": [named[FC1]], "lr": 1e-3})
            topt.add_param_group({"params": [ref[FC1]], "lr": 1e-3})
        given_grads(m, 60 + it)
        copy_grads(m, ref)
        topt.step()
        opt.step()
        w, name = worst(m, ref)
        print("step", it, "worst parameter", w, name)
        assert w <= LIMIT, (it, w, name)
    assert not torch.equal(named[FC1].detach(), fc1)
    assert opt.state_dict()["group_steps"] == [4, 2] and opt.param_groups[1]["weight_decay"] == 0.01


def test_state_dict_round_trip():
    """Three groups and one skipped step; a fresh optimizer on a copy of the model loads the state and continues
    bit-equal to the original for one more step."""
    torch.manual_seed(29)
    ma = toy()
    mb = copy.deepcopy(ma)
    ma, mb = ma.cuda(), mb.cuda()

    def make(m):
        head = list(m.out_layer.parameters())
        gs = decay_groups(m, 0.01, decoupled_weight_decay=True)
        for g in gs:
            g["params"] = [p for p in g["params"] if all(p is not h for h in head)]
        gs[1]["lr"] = 1e-4
        return FusedAdam(m, lr=3e-3, skip_nonfinite=True, max_grad_norm=1.0, fused_zero_grad=True,
                         param_groups=gs + [dict(params=head, lr=1e-3, betas=(0.8, 0.99))])

    oa = make(ma)
    for it in range(3):
        st = given_grads(ma, 70 + it)
        if it == 1:
            st.g(FC2).view(-1)[0] = float("-inf")
        oa.step()
    sd = oa.state_dict()
    assert sd["group_steps"] == [2, 2, 2] and sd["skipped"] == 1 and sd["step"] == 2 and sd["step_calls"] == 3
    mb.load_state_dict(ma.state_dict())
    ob = make(mb)
    ob.load_state_dict(copy.deepcopy(sd))
    assert int(ob.skipped_steps) == 1 and ob.step_count == 3
    for m, o in ((ma, oa), (mb, ob)):
        given_grads(m, 80)
        o.step()
    for (n, pa), (_, pb) in zip(ma.named_parameters(), mb.named_parameters()):
        assert torch.equal(pa.detach(), pb.detach()), n
    assert torch.equal(oa._m, ob._m) and torch.equal(oa._v, ob._v)
    assert ob.state_dict()["group_steps"] == [3, 3, 3] and float(ob.last_grad_norm) == float(oa.last_grad_norm)


@pytest.mark.parametrize("source", ["written before groups existed", "a run without skip_nonfinite", "a run with skip_nonfinite"])
def test_checkpoints_load_across_the_skip_flag(source):
    """torch's load_state_dict takes `fused` and the place of every `step` from the SAVED tail groups.  Whatever wrote the
    checkpoint, a skip_nonfinite optimizer's tail is torch's fused Adam afterwards (one finite and one poisoned step run,
    and the poisoned one changes nothing), and an optimizer without the flag keeps the default Adam; both continue
    within the kernel limit of a torch.optim.Adam that took the same finite steps."""
    torch.manual_seed(37)
    ma = toy()
    mb, mc = copy.deepcopy(ma), copy.deepcopy(ma)
    ma, mb, mc = ma.cuda(), mb.cuda(), mc.cuda()
    ref = clones(ma)
    topt = torch.optim.Adam(list(ref.values()), lr=3e-3, weight_decay=0.01)
    oa = FusedAdam(ma, lr=3e-3, weight_decay=0.01, skip_nonfinite=source.endswith("with skip_nonfinite"))
    for seed in (90, 91):
        given_grads(ma, seed)
        copy_grads(ma, ref)
        topt.step()
        oa.step()
    sd = copy.deepcopy(oa.state_dict())
    if source.startswith("written before"):
        for k in ("group_steps", "skipped", "step_calls"):
            del sd[k]
        del sd["param_groups"][0]["param_names"], sd["param_groups"][0]["decoupled_weight_decay"]
        for g in sd["tail"]["param_groups"]:
            del g["decoupled_weight_decay"]
    for m, skip in ((mb, True), (mc, False)):
        m.load_state_dict(ma.state_dict())
        o = FusedAdam(m, lr=3e-3, weight_decay=0.01, skip_nonfinite=skip, fused_zero_grad=True)
        o.load_state_dict(copy.deepcopy(sd))
        tail = o._tail_opt
        assert all(g["fused"] is (True if skip else None) for g in tail.param_groups)
        assert all(tail.state[p]["step"].is_cuda == skip and float(tail.state[p]["step"]) == 2.0
                   for g in tail.param_groups for p in g["params"])
        assert o.state_dict()["group_steps"] == [2]
        r = {n: t.detach().clone().requires_grad_(True) for n, t in ref.items()}
        t2 = torch.optim.Adam(list(r.values()), lr=3e-3, weight_decay=0.01)
        t2.load_state_dict(copy.deepcopy(topt.state_dict()))
        given_grads(m, 92)
        copy_grads(m, r)
        t2.step()
        o.step()
        w, name = worst(m, r)
        print(source, "-> skip_nonfinite", skip, "worst parameter", w, name)
        assert w <= LIMIT, (skip, w, name)
        if skip:
            before = full_state(m, o)
            st = given_grads(m, 93)
            st.g(FC2).view(-1)[1] = float("nan")
            o.step()
            assert int(o.skipped_steps) == 1 and o.state_dict()["group_steps"] == [3]
            for i, (a, b) in enumerate(zip(before, full_state(m, o))):
                assert torch.equal(a, b), i
