"""No-GPU checks of MultiheadAttention's per-sample masks and biases: the image helper (models/attention.py:
effective_image, a pure function on any device) and the argument checks, which need no device."""
import itertools

import numpy as np
import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd.models import MultiheadAttention
from bpmult_amd.models.attention import effective_image, image_lead

from mha_sample_bias_cases import CASES, FORMS, as4, case, sample_bias

B, H, T, S = 3, 2, 6, 7                       # S % 4 != 0 and T % 4 != 0: both leading dimensions are padded
NINF = float("-inf")
SHAPES = {"TS": (T, S), "HTS": (H, T, S), "11TS": (1, 1, T, S), "1HTS": (1, H, T, S), "B1TS": (B, 1, T, S), "BHTS": (B, H, T, S),
          "(BH)TS": (B * H, T, S)}


def tensor(shape, seed, boolean=False):
    g = torch.Generator().manual_seed(seed)
    if boolean:
        t = torch.rand(shape, generator=g) < 0.3
        t[..., 0] = False
        return t
    t = torch.randn(shape, generator=g)
    t[torch.rand(shape, generator=g) < 0.2] = NINF
    return t


def as_bhts(t):
    """what the forms mean, written out: -> float [Bm, Hm, T, S]"""
    if t.dtype == torch.bool:
        t = torch.where(t, torch.tensor(NINF), torch.tensor(0.0))
    if t.dim() == 2:
        return t[None, None]
    if t.dim() == 3:
        return t[None] if t.shape[0] == H else t.reshape(B, H, T, S)
    return t


BIAS_SHAPES = [f for f in SHAPES if f != "BHTS"]          # a bias per sample and head is passed as [B*H, T, S]: the 4-D spelling stays refused


@pytest.mark.parametrize("mask_form,bias_form,boolean", [(m, b, z) for m, b in itertools.product([None] + list(SHAPES), [None] + BIAS_SHAPES) if m or b
                                                         for z in ((False, True) if m else (False,))])       # only attn_mask may be bool
def test_effective_image_is_the_broadcast_sum(mask_form, bias_form, boolean):
    mask = None if mask_form is None else tensor(SHAPES[mask_form], 1, boolean)
    bias = None if bias_form is None else tensor(SHAPES[bias_form], 2)
    m, mt, ldm, ldt, hs, hst, bs, bst = effective_image(mask, bias, B, H, T, S)
    parts = [as_bhts(t) for t in (mask, bias) if t is not None]
    Bm, Hm = max(p.shape[0] for p in parts), max(p.shape[1] for p in parts)
    want = parts[0].expand(Bm, Hm, T, S).clone()
    if len(parts) == 2:
        want = want + parts[1]
    assert (ldm, ldt) == (8, 8) and m.shape == (Bm, Hm, T, ldm) and mt.shape == (Bm, Hm, S, ldt)
    assert m.dtype == mt.dtype == torch.float32 and m.is_contiguous() and mt.is_contiguous()
    assert torch.equal(m[..., :S], want), "the image is the broadcast sum, smallest common form"
    assert (m[..., S:] == 0).all() and (mt[..., T:] == 0).all(), "pad columns are zeros"
    assert torch.equal(mt[..., :T], want.transpose(2, 3)), "the transpose agrees"
    assert (hs, hst) == ((T * ldm, S * ldt) if Hm > 1 else (0, 0))
    assert (bs, bst) == ((Hm * T * ldm, Hm * S * ldt) if Bm > 1 else (0, 0))
    per_sample = any(f in ("B1TS", "BHTS", "(BH)TS") for f in (mask_form, bias_form))
    per_head = any(f in ("HTS", "1HTS", "BHTS", "(BH)TS") for f in (mask_form, bias_form))
    assert (Bm, Hm) == (B if per_sample else 1, H if per_head else 1)


def test_effective_image_is_not_part_of_the_autograd_graph():
    bias = torch.zeros(B * H, T, S, requires_grad=True) * 2.0
    m, mt, *_ = effective_image(None, bias, B, H, T, S)
    assert not m.requires_grad and not mt.requires_grad


def test_the_reading_of_a_three_dimensional_tensor():
    assert image_lead((H, T, S), B, H, T, S) == (1, H), "leading H: per head, as before"
    assert image_lead((B * H, T, S), B, H, T, S) == (B, H), "leading B*H: torch's flattening, index b*H + h"
    assert image_lead((H, T, S), 1, H, T, S) == (1, H), "B = 1: the two readings coincide"
    assert image_lead((3, T, S), 3, 3, T, S) == (1, 3), "B = H: a leading H keeps the per-head meaning"
    assert image_lead((9, T, S), 3, 3, T, S) == (3, 3)
    img = torch.arange(B * H * T * S, dtype=torch.float32).reshape(B * H, T, S)
    m = effective_image(img, None, B, H, T, S)[0]
    for b in range(B):
        for h in range(H):
            assert torch.equal(m[b, h, :, :S], img[b * H + h])


def test_the_cases_of_the_gpu_tests_are_well_posed():
    """every query row of every sample keeps a visible key (a finite fp64 restatement is asserted on the GPU side too)"""
    for c in CASES:
        for form in FORMS:
            a = as4(c, sample_bias(c, form))
            assert a.shape[0] == c[4] and (~np.isinf(a)).any(-1).all(), (c[0], form)
            assert len({a[b].tobytes() for b in range(a.shape[0])}) == a.shape[0], "one distinct image per sample"


REFUSED = [(4, T, S), (B, T, S), (B * H + 1, T, S), (2, H, T, S), (B, 3, T, S), (H, B, T, S), (T, S + 1), (T + 1, S), (1, 1, 1, T, S), (S,),
           (B, H, S, T)]


@pytest.mark.parametrize("shape", REFUSED)
def test_refused_shapes_raise_before_a_device_is_needed(shape):
    m = MultiheadAttention(8 * H, H)
    q, k = torch.zeros(T, B, 8 * H), torch.zeros(S, B, 8 * H)
    with pytest.raises(ValueError, match=r"attn_bias of shape .*\[T, S\], \[H, T, S\], \[Bm, Hm, T, S\].*\[B\*H, T, S\]"):
        m(q, k, k, attn_bias=torch.zeros(shape))
    for dt in (torch.float32, torch.bool):
        with pytest.raises(ValueError, match=r"attn_mask must be .*\[T, S\], \[H, T, S\], \[Bm, Hm, T, S\].*\[B\*H, T, S\]"):
            m(q, k, k, attn_mask=torch.zeros(shape, dtype=dt))


@pytest.mark.parametrize("form", list(SHAPES))
def test_accepted_shapes_reach_the_device_check(form):
    m = MultiheadAttention(8 * H, H)
    q, k = torch.zeros(T, B, 8 * H), torch.zeros(S, B, 8 * H)
    bias_kw = [dict(attn_bias=torch.zeros(SHAPES[form], requires_grad=True))] if form in BIAS_SHAPES else []
    for kw in bias_kw + [dict(attn_mask=torch.zeros(SHAPES[form])),
               dict(attn_mask=torch.zeros(SHAPES[form], dtype=torch.bool)), dict(attn_mask=torch.zeros(SHAPES[form]), attn_bias=torch.zeros(T, S))]:
        with pytest.raises(RuntimeError, match="no CPU path"):          # valid arguments: only the device is missing
            m(q, k, k, **kw)


def test_the_other_refusals_stand():
    m = MultiheadAttention(8 * H, H)
    q, k = torch.zeros(T, B, 8 * H), torch.zeros(S, B, 8 * H)
    with pytest.raises(ValueError, match="no gradient"):
        m(q, k, k, attn_mask=torch.zeros(B, 1, T, S, requires_grad=True))
    with pytest.raises(ValueError, match="attn_mask must be"):
        m(q, k, k, attn_mask=torch.zeros(B, 1, T, S, dtype=torch.int32))
    with pytest.raises(ValueError, match="float32"):
        m(q, k, k, attn_bias=torch.zeros(B, 1, T, S, dtype=torch.bool))
    m.precision = "bf16x3"
    with pytest.raises(ValueError, match="bf16x3"):
        m(q, k, k, attn_bias=torch.zeros(B * H, T, S))
    m.precision = None
    # the 4-D bias per sample AND head stays refused, as before the per-sample forms (tests/test_mha_bias_cpu.py); the message
    # names the form that takes it
    with pytest.raises(ValueError, match=r"attn_bias of shape \(3, 2, 6, 7\).*\[B\*H, T, S\] = \[6, 6, 7\]"):
        m(q, k, k, attn_bias=torch.zeros(B, H, T, S))
    with pytest.raises(RuntimeError, match="no CPU path"):
        m(q, k, k, attn_bias=torch.zeros(B, H, T, S).reshape(B * H, T, S))
