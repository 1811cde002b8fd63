"""No-GPU checks of the opt-in HIP embeddings of the text encoder (`args.text_embeddings`, models/bert.py): the switch, its
default and its refusals, the untouched state_dict, the sequence-length check that is made from the shapes before the
device check, and host-side argument validation of the two new entry points (rejected calls only: a call that passes
validation launches)."""
import ctypes as C

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib
from bpmult_amd.models import get_model
from bpmult_amd.models.bpmult import BertEncoder
from test_text_encoder_cpu import _args, _save_tiny


@pytest.fixture(scope="module")
def lib():
    _lib.build()
    return _lib.lib()


def test_ctypes_structs_of_the_embedding_entries_mirror_the_header():
    import test_abi_cpu as T
    assert T._c_fields("bpm_bert_embed_problem") == [f[0] for f in _lib.BertEmbedProblem._fields_]
    assert T._c_fields("bpm_bert_scatter_problem") == [f[0] for f in _lib.BertScatterProblem._fields_]
    assert _lib.ABI_VERSION == 5                                  # entries were added, nothing changed


def _valid_embed():
    p = _lib.BertEmbedProblem()
    p.ids, p.seg, p.word, p.pos, p.type = 0x10000, 0x20000, 0x30000, 0x40000, 0x50000
    p.V, p.P, p.Tt, p.gamma, p.beta, p.B, p.L = 60, 64, 2, 0x60000, 0x70000, 3, 37
    p.x, p.xc, p.ldc, p.s, p.mean, p.rstd, p.bad = 0x80000, 0x90000, 64, 0xA0000, 0xB0000, 0xC0000, 0xD0000
    return p


def test_embed_fwd_validates_on_the_host(lib):
    fn = lib.bpm_bert_embed_fwd
    assert fn(_lib.BPM_F32, C.byref(_lib.BertEmbedProblem()), 64, 1e-12, 0, None) == -1      # all-zero problem
    assert fn(_lib.BPM_F32, None, 64, 1e-12, 0, None) == -1
    p = _valid_embed()
    for d in (0, 48, 100, 1056, 2048):                                                       # d % 32, d > 1024
        assert fn(_lib.BPM_F32, C.byref(p), d, 1e-12, 0, None) == -1, d
    assert fn(_lib.BPM_BF16X3, C.byref(p), 64, 1e-12, 0, None) == -1                          # GEMM-only compute type
    p.L = 65                                                                                  # more positions than the table has
    assert fn(_lib.BPM_F32, C.byref(p), 64, 1e-12, 0, None) == -1
    p = _valid_embed()
    p.ldc = 32                                                                                # CT rows shorter than d
    assert fn(_lib.BPM_F32, C.byref(p), 64, 1e-12, 0, None) == -1
    for name in ("word", "pos", "type", "gamma", "beta", "x", "s"):                           # 16-byte rows
        p = _valid_embed()
        setattr(p, name, getattr(p, name) + 4)
        assert fn(_lib.BPM_F32, C.byref(p), 64, 1e-12, 0, None) == -2, name
    p = _valid_embed()
    p.ids += 4                                                                                # int64 ids
    assert fn(_lib.BPM_F32, C.byref(p), 64, 1e-12, 0, None) == -2
    p = _valid_embed()
    p.xc += 4                                                                                 # 8-byte bf16 quads are fine, 4 bytes are not
    assert fn(_lib.BPM_BF16, C.byref(p), 64, 1e-12, 0, None) == -2
    for name in ("ids", "word", "pos", "type", "gamma", "beta", "x", "s", "mean", "rstd", "bad"):
        p = _valid_embed()
        setattr(p, name, None)
        assert fn(_lib.BPM_F32, C.byref(p), 64, 1e-12, 0, None) == -1, name


def _valid_scatter(lib):
    p = _lib.BertScatterProblem()
    p.ds, p.sorted_ids, p.perm, p.seg = 0x10000, 0x20000, 0x30000, 0x40000
    p.dword, p.dpos, p.dtype, p.V, p.Tt, p.B, p.L, p.padding_idx = 0x50000, 0x60000, 0x70000, 60, 2, 3, 37, 0
    p.ws, p.ws_bytes = 0x80000, lib.bpm_bert_embed_scatter_ws_bytes(111, 64, 2)
    return p


def test_embed_scatter_validates_on_the_host(lib):
    fn = lib.bpm_bert_embed_scatter
    assert fn(C.byref(_lib.BertScatterProblem()), 64, None) == -1                             # all-zero problem
    assert fn(None, 64, None) == -1
    for d in (0, 48, 1056):
        assert fn(C.byref(_valid_scatter(lib)), d, None) == -1, d
    p = _valid_scatter(lib)
    p.dword = p.dpos = p.dtype = None                                                         # nothing to compute
    assert fn(C.byref(p), 64, None) == -1
    p = _valid_scatter(lib)
    p.perm = None                                                                             # the word table needs the sorted ids
    assert fn(C.byref(p), 64, None) == -1
    p = _valid_scatter(lib)
    p.ws_bytes -= 4                                                                           # workspace too small
    assert fn(C.byref(p), 64, None) == -1
    for name in ("ds", "dword", "dpos", "dtype", "ws"):
        p = _valid_scatter(lib)
        setattr(p, name, getattr(p, name) + 4)
        assert fn(C.byref(p), 64, None) == -2, name
    # two slots per 32 sorted positions plus one partial row per type id and 32 rows
    assert lib.bpm_bert_embed_scatter_ws_bytes(111, 64, 2) == (2 * 4 + 4 * 2) * 64 * 4
    assert lib.bpm_bert_embed_scatter_ws_bytes(0, 64, 2) == 0


def test_default_is_torch_and_bad_values_raise(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    enc = BertEncoder(_args(bert_model=d, text_features=False))
    assert enc.text_embeddings == "torch" and enc.text_encoder == "torch" and enc.bad_token_ids is None
    assert BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip")).text_embeddings == "torch"
    assert BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip", text_embeddings="hip")).text_embeddings == "hip"
    for bad in ("HIP", "triton", "", None):
        with pytest.raises(ValueError, match="text_embeddings"):
            BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip", text_embeddings=bad))
    with pytest.raises(ValueError, match="needs text_encoder='hip'"):
        BertEncoder(_args(bert_model=d, text_features=False, text_embeddings="hip"))
    with pytest.raises(ValueError, match="needs text_encoder='hip'"):
        get_model(_args(bert_model=d, text_features=False, text_encoder="torch", text_embeddings="hip"))


def test_hidden_size_beyond_the_row_kernels_is_refused(tmp_path):
    wide = _save_tiny(tmp_path / "wide", hidden_size=1056, num_attention_heads=11, intermediate_size=32)
    with pytest.raises(ValueError, match="hidden_size 1056 > 1024"):
        BertEncoder(_args(bert_model=wide, text_features=False, text_encoder="hip", text_embeddings="hip"))
    BertEncoder(_args(bert_model=wide, text_features=False, text_encoder="hip"))             # the layer stack alone takes it


def test_state_dict_and_parameters_are_identical_under_both_settings(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    m_t = get_model(_args(bert_model=d, text_features=False, text_encoder="hip"))
    m_h = get_model(_args(bert_model=d, text_features=False, text_encoder="hip", text_embeddings="hip"))
    assert list(m_t.state_dict()) == list(m_h.state_dict())
    assert [n for n, _ in m_t.named_parameters()] == [n for n, _ in m_h.named_parameters()]
    assert any(k.startswith("enc.bert.embeddings.word_embeddings") for k in m_h.state_dict())
    from transformers import BertModel
    assert type(m_h.enc.bert) is BertModel
    m_h.load_state_dict(m_t.state_dict())


def test_too_many_positions_raise_before_the_device_check(tmp_path):
    d = _save_tiny(tmp_path / "bert")                                       # max_position_embeddings = 32
    enc = BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip", text_embeddings="hip"))
    txt = torch.randint(1, 60, (2, 33))
    with pytest.raises(ValueError, match="max_position_embeddings = 32"):
        enc(txt, torch.ones_like(txt), None)
    txt = torch.randint(1, 60, (2, 32))                                     # L == P passes that check and meets the device check
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc(txt, torch.ones_like(txt), None)


def test_default_setting_dispatches_as_before(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    txt = torch.randint(1, 60, (2, 9))
    enc = BertEncoder(_args(bert_model=d, text_features=False)).eval()
    out = enc(txt, torch.ones_like(txt), torch.zeros_like(txt))
    ref = enc.bert(input_ids=txt, token_type_ids=torch.zeros_like(txt), attention_mask=torch.ones_like(txt), return_dict=False)[0]
    assert torch.equal(out, ref) and enc._embd is None and enc._stack is None
    # text_encoder = "hip" with the default embeddings still computes them on torch and then meets the device check
    enc = BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip"))
    with pytest.raises(RuntimeError, match="no CPU path"):
        enc(txt, torch.ones_like(txt), torch.zeros_like(txt))
    assert enc._embd is None
