"""No-GPU checks of the opt-in HIP text encoder (`args.text_encoder`, models/bert.py): the switch and its default, the
untouched state_dict, the refusals, and host-side argument validation of the new entry points (rejected calls only: a call
that passes validation launches)."""
import ctypes as C
from types import SimpleNamespace

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib
from bpmult_amd.models import get_model
from bpmult_amd.models.bpmult import BertEncoder


def _tiny_cfg(**kw):
    from transformers import BertConfig
    base = dict(vocab_size=60, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                max_position_embeddings=32)
    base.update(kw)
    return BertConfig(**base)


def _save_tiny(path, **kw):
    from transformers import BertModel
    torch.manual_seed(0)
    BertModel(_tiny_cfg(**kw)).save_pretrained(path)
    return str(path)


def _args(**kw):
    a = dict(model="mmtrvat", orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=24, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=1, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0., res_dropout=0.,
             out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6, bert_model="unused", text_features=True,
             num_vectors_l=48, num_vectors_a=48, num_vectors_v=48)
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def test_default_is_torch_and_unknown_values_raise(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    assert BertEncoder(_args()).text_encoder == "torch"
    assert BertEncoder(_args(bert_model=d, text_features=False)).text_encoder == "torch"
    assert BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip")).text_encoder == "hip"
    for bad in ("HIP", "triton", "", None):
        with pytest.raises(ValueError, match="text_encoder"):
            BertEncoder(_args(text_encoder=bad))
    with pytest.raises(ValueError, match="text_encoder"):
        get_model(_args(text_encoder="cuda"))


def test_state_dict_keys_are_identical_under_both_settings(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    m_t = get_model(_args(bert_model=d, text_features=False))
    m_h = get_model(_args(bert_model=d, text_features=False, text_encoder="hip"))
    sd_t, sd_h = m_t.state_dict(), m_h.state_dict()
    assert list(sd_t) == list(sd_h)
    assert any(k.startswith("enc.bert.encoder.layer.1.") for k in sd_h)
    assert [n for n, _ in m_t.named_parameters()] == [n for n, _ in m_h.named_parameters()]
    for k in sd_t:
        if k.startswith("enc.bert."):
            assert torch.equal(sd_t[k], sd_h[k]), k          # both load the same directory


def test_hip_text_encoder_has_no_cpu_path(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    enc = BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip"))
    txt = torch.randint(1, 60, (2, 9))
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc(txt, torch.ones_like(txt), torch.zeros_like(txt))
    # the default setting still runs on the CPU (plain HF)
    out = BertEncoder(_args(bert_model=d, text_features=False))(txt, torch.ones_like(txt), torch.zeros_like(txt))
    assert out.shape == (2, 9, 32)


@pytest.mark.parametrize("kw,what", [(dict(hidden_act="relu"), "hidden_act"), (dict(hidden_act="gelu_new"), "hidden_act"),
                                     (dict(position_embedding_type="relative_key"), "position_embedding_type"),
                                     (dict(is_decoder=True), "is_decoder"),
                                     (dict(add_cross_attention=True, is_decoder=True), "is_decoder"),
                                     (dict(hidden_size=1024, num_attention_heads=2), "head_dim"),
                                     (dict(hidden_size=40, num_attention_heads=2), "multiples of 32"),
                                     (dict(intermediate_size=100), "multiples of 32")])
def test_unsupported_configs_are_refused_at_construction(kw, what):
    from bpmult_amd.models.bert import check_config
    cfg = _tiny_cfg(**kw)
    for k, v in kw.items():                # whatever this transformers version does with the keyword, the refusal reads it
        setattr(cfg, k, v)
    with pytest.raises(ValueError, match=what):
        check_config(cfg)
    check_config(_tiny_cfg())              # the supported configuration passes


def test_unsupported_config_is_refused_by_the_encoder(tmp_path):
    d = _save_tiny(tmp_path / "bert_relu", hidden_act="relu")
    with pytest.raises(ValueError, match="hidden_act"):
        BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip"))
    BertEncoder(_args(bert_model=d, text_features=False))          # the torch setting takes any HF configuration


def _valid_attn():
    a = _lib.AttnProblem()
    a.Q, a.K, a.V, a.O, a.lse = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    a.dO, a.delta, a.dQ, a.dK, a.dV = 0x60000, 0x70000, 0x80000, 0x90000, 0xA0000
    a.ldo = a.lddq = a.lddk = a.lddv = 64
    a.B, a.H, a.T, a.S, a.dh, a.dhp = 2, 1, 5, 5, 64, 64
    a.dq_scale = 1.0
    return a


@pytest.mark.parametrize("name", ["bpm_attn_fwd_kmask", "bpm_attn_bwd_dq_kmask", "bpm_attn_bwd_dkv_kmask"])
def test_kmask_entries_validate_on_the_host(lib, name):
    fn = getattr(lib, name)
    zero, km = _lib.AttnProblem(), _lib.AttnKMask()
    km.mask, km.ldm = 0xB0000, 5
    for dt in (_lib.BPM_F32, _lib.BPM_BF16):
        assert fn(dt, C.byref(zero), C.byref(km), 1, 0, None) == -1            # all-zero problem
        a = _valid_attn()
        null = _lib.AttnKMask()
        null.ldm = 5
        assert fn(dt, C.byref(a), C.byref(null), 1, 0, None) == -1             # null mask pointer on a valid problem
        assert fn(dt, C.byref(a), None, 1, 0, None) == -1                      # no mask array at all
        short = _lib.AttnKMask()
        short.mask, short.ldm = 0xB0000, 4
        assert fn(dt, C.byref(a), C.byref(short), 1, 0, None) == -1            # ldm < S
        assert fn(dt, C.byref(a), C.byref(km), 0, 0, None) == -1               # no problems
        assert fn(dt, None, C.byref(km), 1, 0, None) == -1
    a = _valid_attn()
    assert fn(_lib.BPM_BF16X3, C.byref(a), C.byref(km), 1, 0, None) == -1      # GEMM-only compute type


@pytest.mark.parametrize("name", ["bpm_gelu_fwd", "bpm_gelu_bwd"])
def test_gelu_entries_validate_on_the_host(lib, name):
    fn = getattr(lib, name)
    g = _lib.GeluProblem()
    assert fn(_lib.BPM_F32, C.byref(g), 1, None) == -1                         # all-zero problem
    assert fn(_lib.BPM_F32, None, 1, None) == -1
    g.u, g.ldu, g.g, g.ldg, g.dg, g.lddg, g.du, g.lddu, g.R, g.C = 0x10000, 64, 0x20000, 64, 0x30000, 64, 0x40000, 64, 3, 64
    assert fn(_lib.BPM_F32, C.byref(g), 0, None) == -1
    assert fn(_lib.BPM_F32, C.byref(g), _lib.MAX_GROUP + 1, None) == -1
    assert fn(_lib.BPM_BF16X3, C.byref(g), 1, None) == -1
    g.ldu = 66
    assert fn(_lib.BPM_F32, C.byref(g), 1, None) == -2                         # rows that are not whole 4-element chunks
    g.ldu, g.ldg, g.lddu = 64, 60, 60
    assert fn(_lib.BPM_F32, C.byref(g), 1, None) == -1                         # output rows shorter than C
    g.ldg, g.lddu, g.u = 64, 64, 0x10004
    assert fn(_lib.BPM_F32, C.byref(g), 1, None) == -2                         # misaligned input


def test_ctypes_structs_of_the_new_entries_mirror_the_header():
    import test_abi_cpu as T
    assert T._c_fields("bpm_attn_kmask") == [f[0] for f in _lib.AttnKMask._fields_]
    assert T._c_fields("bpm_gelu_problem") == [f[0] for f in _lib.GeluProblem._fields_]
