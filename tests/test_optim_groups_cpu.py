"""No-GPU checks of FusedAdam's parameter groups: the new struct mirrors the header, bpm_adam_step_groups validates its
arguments on the host before anything is launched, the constructor's rules, optim.decay_groups, the grouped segment
table of the toy store (built from host tensors under ops._DRY_RUN) and the state-dict format."""
import ctypes as C
import os
import re
from types import SimpleNamespace

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, ops
from bpmult_amd.optim import FusedAdam, decay_groups

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEADER = open(os.path.join(ROOT, "include", "bpmult_hip.h")).read()


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def _c_fields(struct_name):
    body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (struct_name, struct_name), HEADER, flags=re.S).group(1)
    body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
    names = []
    for decl in body.split(";"):
        decl = decl.strip()
        if not decl:
            continue
        parts = decl.split(",")
        names.append(parts[0].split()[-1].lstrip("*"))
        names += [p.strip().lstrip("*") for p in parts[1:]]
    return [re.sub(r"\[\d+\]$", "", n) for n in names]


def test_structs_mirror_the_header():
    assert _c_fields("bpm_adam_group") == [f[0] for f in _lib.AdamGroup._fields_]
    assert _c_fields("bpm_adam_group") == ["lr", "beta1", "beta2", "eps", "weight_decay", "decoupled", "step", "pad_"]
    assert C.sizeof(_lib.AdamGroup) == 32
    assert _c_fields("bpm_adam_seg") == [f[0] for f in _lib.AdamSeg._fields_]
    assert _c_fields("bpm_adam_seg")[-1] == "group" and C.sizeof(_lib.AdamSeg) == 40
    assert _lib.ADAM_MAX_GROUPS == int(re.search(r"#define BPM_ADAM_MAX_GROUPS (\d+)", HEADER).group(1)) == 16
    assert _lib.ABI_VERSION == int(re.search(r"#define BPM_ABI_VERSION (\d+)", HEADER).group(1)) == 5


def test_the_new_entry_validates_on_the_host(lib):
    """Made-up aligned addresses: only rejected calls are made here (a call that passes validation launches)."""
    tab, p, g, m, v, dev = 0x10000, 0x50000, 0x60000, 0x70000, 0x80000, 0x90000
    one = ops.adam_groups([dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=0., step=1)])
    assert one[0].step == 1 and one[0].decoupled == 0 and abs(one[0].beta2 - .999) < 1e-7

    def call(table=tab, nseg=1, nblk=1, param=p, grad=g, ea=m, eas=v, groups=one, ngroups=1, scale=None, norm=None, steps=None,
             skipped=None):
        return lib.bpm_adam_step_groups(_lib.BPM_F32, table, nseg, nblk, param, grad, ea, eas, groups, ngroups, 1.0, scale, norm,
                                        steps, skipped, 0, None)

    assert call(table=None) == -1 and call(nseg=0) == -1 and call(nblk=0) == -1
    assert call(param=None) == -1 and call(grad=None) == -1 and call(ea=None) == -1 and call(eas=None) == -1
    assert call(groups=None) == -1
    assert call(ngroups=0) == -1 and call(ngroups=17) == -1 and call(ngroups=-1) == -1
    for k in ("param", "grad", "ea", "eas"):
        assert call(**{k: 0x50004}) == -2, k                                   # the four buffers: 16 bytes
        assert call(**{k: 0x50008}) == -2, k
    for k in ("scale", "norm", "steps", "skipped"):
        assert call(**{k: dev + 2}) == -2, k                                   # the device scalars: 4 bytes
    zero = ops.adam_groups([dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=0., step=0)])
    assert call(groups=zero) == -1                                             # host step >= 1 when steps_dev is NULL
    two = ops.adam_groups([dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=0., step=3),
                           dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=.1, decoupled_weight_decay=True)])
    assert two[1].decoupled == 1 and two[1].step == 0
    assert call(groups=two, ngroups=2) == -1                                   # ... for every group
    with pytest.raises(ValueError, match="groups"):
        ops.adam_groups([])
    with pytest.raises(ValueError, match="groups"):
        ops.adam_groups([dict(lr=1e-3, betas=(.9, .999), eps=1e-8, weight_decay=0.)] * 17)


def _toy(**kw):
    from bpmult_amd.models import get_model
    a = dict(model="mmtrvat", orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=24, vonly=True, lonly=True,
             aonly=True, num_heads=4, layers=1, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.,
             res_dropout=0., out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6,
             bert_model="unused", text_features=True)
    a.update(kw)
    return get_model(SimpleNamespace(**a))


FC1 = "trans_l_with_a.layers.0.fc1.weight"


def test_constructor_validation():
    m = _toy()
    named = dict(m.named_parameters())
    ps = list(m.parameters())
    with pytest.raises(ValueError, match="not a parameter of the model"):
        FusedAdam(m, param_groups=[{"params": [torch.nn.Parameter(named[FC1].detach().clone())]}])      # equal, not identical
    third = list(named)[2]
    with pytest.raises(ValueError, match=re.escape(third) + r".*more than one"):
        FusedAdam(m, param_groups=[{"params": ps[:5]}, {"params": [ps[7], ps[2]]}])
    with pytest.raises(ValueError, match=re.escape(third) + r".*more than one"):
        FusedAdam(m, param_groups=[{"params": [ps[2], ps[3], ps[2]]}])
    with pytest.raises(ValueError, match="group 1 is empty"):
        FusedAdam(m, param_groups=[{"params": ps[:5]}, {"params": []}])
    with pytest.raises(ValueError, match="16"):
        FusedAdam(m, param_groups=[{"params": [p]} for p in ps[:17]])
    named[FC1].requires_grad_(False)
    with pytest.raises(ValueError, match=re.escape(FC1) + r".*requires_grad"):
        FusedAdam(m, param_groups=[{"params": [named[FC1]]}])
    # the default form leaves a frozen parameter out instead
    opt = FusedAdam(m, lr=1e-3)
    assert len(opt.param_groups) == 1 and all(p is not named[FC1] for p in opt.param_groups[0]["params"])
    assert len(opt.param_groups[0]["params"]) == len(ps) - 1
    # add_param_group: the same rules, and the unfreeze-later use
    with pytest.raises(ValueError, match="requires_grad"):
        opt.add_param_group({"params": [named[FC1]]})
    with pytest.raises(ValueError, match="more than one"):
        opt.add_param_group({"params": [ps[-1]]})
    named[FC1].requires_grad_(True)
    opt.add_param_group({"params": [named[FC1]], "lr": 5e-5})
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["lr"] == 5e-5 and opt.param_groups[1]["betas"] == (0.9, 0.999)
    assert opt._group_steps == [0, 0]
    full = FusedAdam(m, param_groups=[{"params": [p]} for p in ps[:16]])
    with pytest.raises(ValueError, match="16"):
        full.add_param_group({"params": [ps[16]]})


@pytest.mark.filterwarnings("ignore:Detected call of `lr_scheduler.step")
def test_defaults_flow_into_the_groups():
    m = _toy()
    ps = list(m.parameters())
    opt = FusedAdam(m, lr=2e-3, betas=(0.8, 0.99), eps=1e-7, weight_decay=0.02, decoupled_weight_decay=True, max_grad_norm=0.8,
                    param_groups=[{"params": ps[:3]}, {"params": ps[3:5], "lr": 1e-4, "betas": [0.7, 0.9], "decoupled_weight_decay": False},
                                  {"params": ps[5:6], "weight_decay": 0.0, "eps": 1e-6}])
    g0, g1, g2 = opt.param_groups
    assert (g0["lr"], g0["betas"], g0["eps"], g0["weight_decay"], g0["decoupled_weight_decay"]) == (2e-3, (0.8, 0.99), 1e-7, 0.02, True)
    assert (g1["lr"], g1["betas"], g1["eps"], g1["weight_decay"], g1["decoupled_weight_decay"]) == (1e-4, (0.7, 0.9), 1e-7, 0.02, False)
    assert (g2["lr"], g2["betas"], g2["eps"], g2["weight_decay"], g2["decoupled_weight_decay"]) == (2e-3, (0.8, 0.99), 1e-6, 0.0, True)
    assert g0["max_grad_norm"] == 0.8
    # one lambda per group has something to act on
    sched = torch.optim.lr_scheduler.LambdaLR(opt, [lambda e: 0.5 ** e, lambda e: 1.0, lambda e: 0.1 ** e])
    sched.step()
    assert abs(g0["lr"] - 1e-3) < 1e-12 and g1["lr"] == 1e-4 and abs(g2["lr"] - 2e-4) < 1e-12
    # the default construction is still one group of every trainable parameter
    d = FusedAdam(m)
    assert len(d.param_groups) == 1 and len(d.param_groups[0]["params"]) == len(ps)
    assert d.param_groups[0]["decoupled_weight_decay"] is False and d.skip_nonfinite is False


def test_decay_groups():
    m = _toy()
    frozen = dict(m.named_parameters())[FC1]
    frozen.requires_grad_(False)
    m.out_layer.bias.requires_grad_(False)
    gs = decay_groups(m, 0.05, lr=3e-4, decoupled_weight_decay=True)
    assert len(gs) == 2
    assert gs[0]["weight_decay"] == 0.05 and gs[1]["weight_decay"] == 0.0
    assert all(g["lr"] == 3e-4 and g["decoupled_weight_decay"] is True for g in gs)
    assert gs[0]["params"] and all(p.ndim >= 2 for p in gs[0]["params"])
    assert gs[1]["params"] and all(p.ndim <= 1 for p in gs[1]["params"])
    got = [id(p) for g in gs for p in g["params"]]
    want = [id(p) for p in m.parameters() if p.requires_grad]
    assert len(got) == len(set(got)) and set(got) == set(want)
    assert id(frozen) not in got and id(m.out_layer.bias) not in got
    opt = FusedAdam(m, lr=1e-3, param_groups=gs)
    assert len(opt.param_groups) == 2 and opt.param_groups[1]["weight_decay"] == 0.0


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    try:
        yield
    finally:
        ops._DRY_RUN = False


def _segments(table, nseg):
    raw = bytes(table.numpy().tobytes())
    assert len(raw) == nseg * C.sizeof(_lib.AdamSeg)
    return list((_lib.AdamSeg * nseg).from_buffer_copy(raw))


def test_grouped_table_of_the_toy_store(dry_run):
    """Three groups (matrices by encoder, then every vector) and two parameters in none: one with a plain shadow, one
    LayerNorm weight."""
    m = _toy()
    st = m._ensure_store()
    m._trunk_for(2)
    plain = st._adam_plain
    ln = next(n for n in st.names if "layer_norm" in n and n.endswith("weight"))
    assert FC1 in plain and ln not in plain and len(plain) > 10
    group_of = {}
    for n in st.names:
        if n in (FC1, ln):
            continue
        p = st.params[n]
        group_of[n] = 2 if p.ndim <= 1 else (0 if n.startswith("trans_l") else 1)
    assert {0, 1, 2} == set(group_of.values())
    tab, nseg, nblk = st.adam_group_table(group_of)
    again = st.adam_group_table(dict(group_of, **{FC1: -1}))                                        # absent == -1
    assert again[1:] == (nseg, nblk) and torch.equal(again[0], tab)
    segs = _segments(tab, nseg)
    # contiguous from 0 to total, 16-byte aligned cuts, blk0 consistent with adam_blocks
    off4, blk = 0, 0
    for s in segs:
        assert s.off4 == off4 and s.blk0 == blk and s.n4 > 0 and (4 * s.off4) % 64 == 0
        off4 += s.n4
        blk += ops.adam_blocks(s.n4)
    assert 4 * off4 == st.total and blk == nblk
    # one group per segment: every parameter lies inside exactly one segment, whose group is the parameter's
    starts = [4 * s.off4 for s in segs]
    own = {}
    for n in st.names:
        a = st.off[n]
        b = a + (st.params[n].numel() + st.ALIGN - 1) // st.ALIGN * st.ALIGN          # the padding rides with its parameter
        hit = [s for s, s0 in zip(segs, starts) if s0 <= a and b <= s0 + 4 * s.n4]
        assert len(hit) == 1, n
        assert hit[0].group == group_of.get(n, -1), n
        own[n] = hit[0]
    # plain-shadow parameters keep a segment of their own, with their shadow; runs carry none
    esz = 2 if st.dtype == _lib.BPM_BF16 else 4
    for n, (rows, cols, dst_ld, off) in plain.items():
        s = own[n]
        assert 4 * s.off4 == st.off[n] and 4 * s.n4 == (st.params[n].numel() + 63) // 64 * 64
        assert (s.dst, s.rows, s.cols, s.dst_ld) == (st.shadow_flat.data_ptr() + esz * off, rows, cols, dst_ld)
    assert sum(1 for s in segs if s.dst) == len(plain)
    assert own[FC1].group == -1 and own[ln].group == -1
    assert 4 * own[ln].off4 == st.off[ln] and 4 * own[ln].n4 == 64                 # cut out of its run on both sides
    # the table of the ungrouped entries is the same walk with every segment in group 0, and has fewer cuts
    base = _segments(st._adam_table[0], st._adam_table[1])
    assert all(s.group == 0 for s in base) and len(base) < nseg and st._adam_table[2] <= nblk
    assert sum(s.n4 for s in base) * 4 == st.total


def test_groups_of_tail_parameters_alone_are_rejected(dry_run):
    """Known once the store exists (it says which parameters are the trunk's): at the first use, with a clear message."""
    m = _toy()
    opt = FusedAdam(m, lr=1e-3, max_grad_norm=0.8, param_groups=[{"params": list(m.out_layer.parameters())}])
    with pytest.raises(ValueError, match="no parameter of the flat trunk buffers"):
        opt.state_dict()


def test_skip_nonfinite_is_fixed_at_construction():
    opt = FusedAdam(_toy(), skip_nonfinite=True)
    assert opt.skip_nonfinite is True
    with pytest.raises(AttributeError):
        opt.skip_nonfinite = False


def test_state_dict_format(dry_run):
    m = _toy()
    named = dict(m.named_parameters())
    ps = list(m.parameters())
    rest = [p for p in ps if p is not named[FC1] and p is not m.out_layer.bias]

    def make():
        return FusedAdam(m, lr=1e-3, max_grad_norm=0.8,
                         param_groups=[{"params": rest, "weight_decay": 0.01}, {"params": [named[FC1]], "lr": 5e-5, "decoupled_weight_decay": True},
                                       {"params": [m.out_layer.bias], "betas": (0.8, 0.99)}])

    opt = make()
    opt._group_steps = [7, 5, 2]
    opt.step_count = 9
    sd = opt.state_dict()
    assert sd["step"] == 7 and sd["group_steps"] == [7, 5, 2] and sd["skipped"] == 0 and sd["step_calls"] == 9
    assert [g["param_names"] for g in sd["param_groups"]][1:] == [[FC1], ["out_layer.bias"]]
    assert len(sd["param_groups"][0]["param_names"]) == len(rest) and "params" not in sd["param_groups"][0]
    assert sd["param_groups"][1]["lr"] == 5e-5 and sd["param_groups"][1]["decoupled_weight_decay"] is True
    assert sd["param_groups"][2]["betas"] == (0.8, 0.99) and sd["param_groups"][0]["max_grad_norm"] == 0.8
    sd["param_groups"][1]["lr"] = 2.5e-5
    sd["param_groups"][2]["betas"] = [0.7, 0.9]                                 # a list, as a JSON round trip leaves it
    new = make()
    new.load_state_dict(sd)
    assert new._group_steps == [7, 5, 2] and new.step_count == 9
    assert new.param_groups[1]["lr"] == 2.5e-5 and new.param_groups[2]["betas"] == (0.7, 0.9)
    assert new.state_dict()["group_steps"] == [7, 5, 2]
    # a checkpoint written before groups existed: no names, no group_steps -- every group takes "step"
    one = FusedAdam(m, lr=1e-3)
    old = one.state_dict()
    for k in ("group_steps", "skipped", "step_calls"):
        del old[k]
    del old["param_groups"][0]["param_names"], old["param_groups"][0]["decoupled_weight_decay"]
    old["step"] = 11
    one.load_state_dict(old)
    assert one._group_steps == [11] and one.step_count == 11 and one.param_groups[0]["decoupled_weight_decay"] is False
    # mismatches
    with pytest.raises(ValueError, match="parameter groups"):
        new.load_state_dict(old)
    bad = make().state_dict()
    bad["param_groups"][1]["param_names"] = ["out_layer.weight"]
    with pytest.raises(ValueError, match="group 1"):
        new.load_state_dict(bad)
    bad = make().state_dict()
    bad["group_steps"] = [1, 2]
    with pytest.raises(ValueError, match="step counts"):
        new.load_state_dict(bad)
