"""No-GPU checks of the encoder's padding masks (TransformerEncoder.forward(..., encoder_padding_mask=, key_padding_mask=)):
the argument checks, which run before anything needs a device; the launch tables, built from HOST tensors (ops._DRY_RUN,
the recording method of test_plan_tables_cpu.py); and the fixture's contents.

Launch tables: tests/golden/encoder_plan_steps.json holds, for one small shape per layer kind and call form, the step
sequence (stream tag and launch function of every step) of the forward and backward tables as the engine built them
BEFORE it knew of masks (recorded from that commit by `trace` below).  A plan built without masks must still build
exactly those; a masked plan the same sequence with the *_kmask entries at the attention steps (bpm_attn_bwd's two
passes as two steps), one mask per problem, and no low-rank key side."""
import json
import os

import numpy as np
import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import engine, ops
from bpmult_amd.models.encoder import TransformerEncoder
from encoder_kpm_cases import CASES, LAYERS, blocks, case, inputs, padding

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLDEN = os.path.join(ROOT, "tests", "golden")


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    try:
        yield
    finally:
        ops._DRY_RUN = False


# --- argument checks -----------------------------------------------------------------------------------------------------
def _enc(bi=False):
    return TransformerEncoder(24, 4, 2, attn_mask=True, biprojection=bi)


X, KV = torch.zeros(3, 2, 24), torch.zeros(5, 2, 24)          # T = 3, S = 5, B = 2


def test_wrong_shape():
    m = _enc()
    with pytest.raises(ValueError, match=r"key_padding_mask of shape \(2, 6\), expected \[2, 5\]"):
        m(X, KV, KV, key_padding_mask=torch.zeros(2, 6, dtype=torch.bool))
    with pytest.raises(ValueError, match="key_padding_mask of shape"):
        m(X, KV, KV, key_padding_mask=torch.zeros(5, 2, dtype=torch.uint8))      # [S, B]
    with pytest.raises(ValueError, match=r"key_padding_mask of shape \(2, 3\), expected \[2, 5\]"):
        m(X, KV, KV, key_padding_mask=torch.zeros(2, 3, dtype=torch.bool))      # x_in's length
    with pytest.raises(ValueError, match=r"encoder_padding_mask of shape \(2, 5\), expected \[2, 3\]"):
        m(X, encoder_padding_mask=torch.zeros(2, 5, dtype=torch.bool))
    with pytest.raises(ValueError, match=r"encoder_padding_mask of shape \(3, 2\), expected \[2, 3\]"):
        _enc(True)(X, KV, KV, encoder_padding_mask=torch.zeros(3, 2, dtype=torch.bool))


def test_float_dtype():
    m = _enc(True)
    for bad in (torch.zeros(2, 5), torch.zeros(2, 5, dtype=torch.int64), [[0] * 5] * 2, torch.zeros(2, 5, requires_grad=True)):
        with pytest.raises(ValueError, match="key_padding_mask must be a torch.bool or torch.uint8 tensor"):
            m(X, KV, KV, key_padding_mask=bad)
    with pytest.raises(ValueError, match="encoder_padding_mask must be a torch.bool or torch.uint8 tensor"):
        m(X, encoder_padding_mask=torch.zeros(2, 3))
    with pytest.raises(ValueError, match="encoder_padding_mask must be"):
        m(X, KV, KV, encoder_padding_mask=torch.zeros(2, 3, dtype=torch.float64), key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))


def test_mask_on_another_device():
    m = _enc(True)
    with pytest.raises(ValueError, match="key_padding_mask on meta, the inputs on cpu"):
        m(X, KV, KV, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool, device="meta"))
    with pytest.raises(ValueError, match="encoder_padding_mask on meta, the inputs on cpu"):
        m(X, encoder_padding_mask=torch.zeros(2, 3, dtype=torch.uint8, device="meta"))


@pytest.mark.parametrize("bi", [False, True])
def test_key_padding_mask_in_the_self_attention_form(bi):
    m = _enc(bi)
    ok = torch.zeros(2, 3, dtype=torch.bool)
    with pytest.raises(ValueError, match="key_padding_mask .* self-attention call form has no key source"):
        m(X, key_padding_mask=ok)
    with pytest.raises(ValueError, match="self-attention call form has no key source"):
        m(X, None, KV, key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))      # one of k / v missing: the self form
    with pytest.raises(ValueError, match="self-attention call form has no key source"):
        m(X, encoder_padding_mask=ok, key_padding_mask=ok)


def test_encoder_padding_mask_in_the_plain_crossmodal_form():
    with pytest.raises(ValueError, match="encoder_padding_mask .* no self-attention block"):
        _enc(False)(X, KV, KV, encoder_padding_mask=torch.zeros(2, 3, dtype=torch.bool))
    with pytest.raises(ValueError, match="no self-attention block"):
        _enc(False)(X, KV, KV, encoder_padding_mask=torch.zeros(2, 3, dtype=torch.bool),
                    key_padding_mask=torch.zeros(2, 5, dtype=torch.bool))


def test_the_masks_are_keyword_only():
    with pytest.raises(TypeError):
        _enc(True)(X, KV, KV, torch.zeros(2, 3, dtype=torch.bool))


# --- launch tables -------------------------------------------------------------------------------------------------------
# (name, biprojection, call form, T, S, B, d, H): the kinds and forms of e1 - e5 at their smallest, and a crossmodal shape
# with two query time steps, whose unmasked plan takes the low-rank key side
SHAPES = (("cross", False, "cross", 7, 9, 3, 24, 4), ("bicross", True, "cross", 8, 5, 2, 24, 4), ("self", False, "self", 9, 9, 3, 24, 4),
          ("biself", True, "self", 7, 7, 2, 24, 4), ("lowrank", False, "cross", 2, 8, 2, 24, 2))
UNMASK = {"attn_fwd_kmask": "attn_fwd", "attn_bwd_dq_kmask": "attn_bwd_dq", "attn_bwd_dkv_kmask": "attn_bwd_dkv"}


def _step(s):
    if s is engine.JOIN:
        return "join"
    if s[0] in (engine.MARK, engine.WAIT):
        return f"{s[0]}:{s[1]}"
    if s[0] in (engine.SIDE, engine.SIDE2):
        return f"{s[0]}:{s[1][0].__name__}"
    return s[0].__name__


def trace(plan):
    """{table: [step, ...]}: every step of the plan's forward and backward tables as '<stream tag>:<launch function>'."""
    out = {f"fwd.{int(t)}": [_step(s) for s in plan._fwd[t]] for t in (True, False)}
    out.update({f"bwd.{int(t)}.{int(f)}": [_step(s) for s in plan._bwd[(t, f)]] for t in (True, False) for f in (True, False)})
    return out


def _plans(name, bi, form, Tn, S, B, d, H):
    enc = TransformerEncoder(d, H, LAYERS, attn_dropout=0.1, relu_dropout=0.1, res_dropout=0.1, embed_dropout=0.1, attn_mask=True,
                             biprojection=bi)
    enc.precision = "bf16"
    enc._ensure_store()
    x, kv = torch.zeros(Tn, B, d), (torch.zeros(S, B, d) if form == "cross" else None)
    return enc, x, kv


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_unmasked_plan_builds_the_tables_it_always_built(dry_run, shape):
    want = json.load(open(os.path.join(GOLDEN, "encoder_plan_steps.json")))[shape[0]]
    enc, x, kv = _plans(*shape)
    plan = enc._plan_for(x, kv)
    form, Tn, S, B = shape[2], shape[3], shape[4], shape[5]
    assert list(enc._plans) == [("self", Tn, B) if form == "self" else (Tn, S, B)], "a call without masks reaches its old key"
    assert plan._lowrank == (shape[0] == "lowrank")
    assert trace(plan) == want              # (up to here the test passes on the commit the sequences were recorded from)
    assert plan is enc._plan_for(x, kv, False, False)
    assert not plan._masked and plan._km_self is None and plan._km_cross is None
    assert not any(k.startswith("vis_") for k in plan.buf[0])


@pytest.mark.parametrize("shape", SHAPES, ids=[s[0] for s in SHAPES])
def test_masked_plan_takes_the_kmask_entries_at_the_attention_steps(dry_run, shape):
    want = json.load(open(os.path.join(GOLDEN, "encoder_plan_steps.json")))[shape[0]]
    name, bi, form, Tn, S, B, d, H = shape
    enc, x, kv = _plans(*shape)
    has_self, has_cross = form == "self" or bi, form == "cross"
    combos = [(e, k) for e in ((False, True) if has_self else (False,)) for k in ((False, True) if has_cross else (False,)) if e or k]
    plain = enc._plan_for(x, kv)
    seen = {id(plain)}
    for epm, kpm in combos:
        plan = enc._plan_for(x, kv, epm, kpm)
        assert id(plan) not in seen and plan is enc._plan_for(x, kv, epm, kpm), "keyed by which masks the call carries"
        seen.add(id(plan))
        assert plan._masked and not plan._lowrank
        (b,) = plan.buf
        for nm, n, there in (("vis_s", Tn, has_self), ("vis_c", S, has_cross)):
            assert (nm in b) == there
            if there:                      # uint8, nonzero = visible, contiguous; all ones until a forward fills it
                assert b[nm].dtype == torch.uint8 and b[nm].shape == (B, n) and b[nm].is_contiguous() and bool(b[nm].all())
                assert b[nm].data_ptr() == b[nm + "_b"].data_ptr()
        got = trace(plan)
        if name == "lowrank":
            continue                       # compared with the dK / dV route below
        for tab, steps in got.items():
            # bpm_attn_bwd (the self block's dQ pass, then its dK / dV pass) becomes its two masked passes, in that order
            merged = []
            for s in steps:
                if s == "attn_bwd_dkv_kmask" and merged and merged[-1] == "attn_bwd_dq_kmask" and want[tab][len(merged) - 1] == "attn_bwd":
                    merged[-1] = "attn_bwd"
                    continue
                merged.append(s)
            back = [":".join(UNMASK.get(p, p) for p in s.split(":")) for s in merged]
            assert back == want[tab], tab
            assert not any(s.split(":")[-1] in ("attn_fwd", "attn_bwd", "attn_bwd_dq", "attn_bwd_dkv") for s in steps), tab
        # one mask per problem, pointing at the plan's buffers: the self block's keys are ks (beside a cross block) or kh
        self_k = {t.data_ptr() for t in b["ks" if form == "cross" else "kh"]} if has_self else set()
        n_masked = 0
        for steps in (*plan._fwd.values(), *plan._bwd.values()):
            for s in steps:
                s = s[1] if isinstance(s, tuple) and s[0] in (engine.SIDE, engine.SIDE2) else s
                if isinstance(s, tuple) and s[0] in (ops.attn_fwd_kmask, ops.attn_bwd_dq_kmask, ops.attn_bwd_dkv_kmask):
                    probs, km = s[2], s[3]
                    assert len(km) == len(probs) == 1
                    vis = b["vis_s"] if probs[0].K in self_k else b["vis_c"]
                    assert km[0].mask == vis.data_ptr() and km[0].ldm == vis.shape[1] == probs[0].S
                    n_masked += 1
        # per layer and block: one forward step in each of 2 tables, a dQ and a dK / dV step in each of 4
        assert n_masked == LAYERS * (has_self + has_cross) * (2 + 2 * 4)


def test_masked_plan_has_no_low_rank_key_side(dry_run):
    """Two query time steps: the unmasked crossmodal plan runs its key side low-rank (dS / Pd exported by the dQ pass); the
    masked dQ entry has no such export, so the masked plan takes the dK / dV route."""
    enc, x, kv = _plans(*SHAPES[-1])
    plain, masked = enc._plan_for(x, kv), enc._plan_for(x, kv, False, True)
    assert plain._lowrank and not masked._lowrank
    assert "dSall" in plain.buf[0] and "dSall" not in masked.buf[0] and masked.buf[0]["dkall"] is not None
    names = [s.split(":")[-1] for s in trace(masked)["bwd.1.0"]]
    assert names.count("attn_bwd_dq_kmask") == LAYERS and names.count("attn_bwd_dkv_kmask") == LAYERS and "expand_heads" not in names
    for steps in masked._bwd.values():
        for s in steps:
            s = s[1] if isinstance(s, tuple) and s[0] in (engine.SIDE, engine.SIDE2) else s
            if isinstance(s, tuple) and s[0] is ops.attn_bwd_dq_kmask:
                assert not s[2][0].dS and not s[2][0].Pd


def test_engine_refusals(dry_run):
    d, H, B = 24, 4, 2
    enc = TransformerEncoder(d, H, LAYERS, attn_mask=True, biprojection=True)
    st = enc._ensure_store()
    M = engine.EncoderMasks
    mk = lambda cfg, desc, masks: engine.EncoderGroupPlan(st, cfg, [desc], B, masks=masks)
    with pytest.raises(ValueError, match="tail_rows or a gathered query subset"):
        mk(enc.group_cfg(), engine.EncoderDesc("", 0, 6, 5, 0.0, tail_rows=True), [M(cross_keys=True)])
    with pytest.raises(ValueError, match="no key / value source"):
        mk(enc.group_cfg(self_only=True), engine.EncoderDesc("", 0, 6, 6, 0.0), [M(cross_keys=True)])
    with pytest.raises(ValueError, match="one entry per encoder"):
        mk(enc.group_cfg(), engine.EncoderDesc("", 0, 6, 5, 0.0), [M(), M()])
    plain = TransformerEncoder(d, H, LAYERS, attn_mask=True)
    st2 = plain._ensure_store()
    with pytest.raises(ValueError, match="gathered query subset"):
        engine.EncoderGroupPlan(st2, plain.group_cfg(), [engine.EncoderDesc("", 0, 2, 8, 0.0, q_pos0=0, q_stride=7, T_full=8)], B,
                                masks=[M(cross_keys=True)])
    with pytest.raises(ValueError, match="no self-attention block"):
        engine.EncoderGroupPlan(st2, plain.group_cfg(), [engine.EncoderDesc("", 0, 6, 5, 0.0)], B, masks=[M(self_keys=True)])
    # a masked plan takes exactly the masks it was built for; an unmasked one none
    plan = mk(enc.group_cfg(), engine.EncoderDesc("", 0, 6, 5, 0.0), [M(cross_keys=True)])
    x, kv = torch.zeros(6, B, d), torch.zeros(5, B, d)
    with pytest.raises(ValueError, match="built with a cross-attention key mask, the call comes without one"):
        plan.forward([x], [kv], [kv], 1, True)
    with pytest.raises(ValueError, match="built without a self-attention key mask, the call comes with one"):
        plan.forward([x], [kv], [kv], 1, True, self_masks=[torch.zeros(B, 6, dtype=torch.bool)], cross_masks=[torch.zeros(B, 5, dtype=torch.bool)])
    with pytest.raises(ValueError, match=r"cross-attention key mask must be bool / uint8 \[2,5\]"):
        plan.forward([x], [kv], [kv], 1, True, cross_masks=[torch.zeros(B, 6, dtype=torch.bool)])
    unmasked = engine.EncoderGroupPlan(st, enc.group_cfg(), [engine.EncoderDesc("", 0, 6, 5, 0.0)], B)
    with pytest.raises(ValueError, match="built without a cross-attention key mask"):
        unmasked.forward([x], [kv], [kv], 1, True, cross_masks=[torch.zeros(B, 5, dtype=torch.bool)])


# --- the fixture ---------------------------------------------------------------------------------------------------------
def test_the_fixture_holds_the_cases():
    g = dict(np.load(os.path.join(GOLDEN, "encoder_kpm.npz")))
    assert sorted({k.split(".")[0] for k in g}) == [c[0] for c in CASES] == ["e1", "e2", "e3", "e4", "e5"]
    for c in CASES:
        tag, form, bi, Tn, S, B, d = c[:7]
        assert g[f"{tag}.y"].shape == g[f"{tag}.gx"].shape == (Tn, B, d)
        assert all(np.isfinite(v).all() for k, v in g.items() if k.startswith(tag + "."))
        epm, kpm = padding(c)
        if form == "cross":
            assert g[f"{tag}.gkv"].shape == (S, B, d)
            assert (g[f"{tag}.gkv"][kpm.T] == 0).all(), "d(key source) of a padded position is exactly 0 in the reference's run too"
            assert g[f"{tag}.gkv"][~kpm.T].any()
        else:
            assert f"{tag}.gkv" not in g
        enc = TransformerEncoder(d, c[7], LAYERS, biprojection=bi)
        have = {k[len(tag) + 3:] for k in g if k.startswith(tag + ".g.")}
        unused = {f"layers.{i}.layer_norms.1.{w}" for i in range(LAYERS) for w in ("weight", "bias")} if bi and form == "self" else set()
        assert have == {k for k, _ in enc.named_parameters()} - unused
        assert set(inputs(c)) == ({"x", "kv", "w"} if form == "cross" else {"x", "w"})
    assert [b for b, _ in blocks(case("e3"))] == ["self", "cross"] and all(pm is not None for _, pm in blocks(case("e3")))
