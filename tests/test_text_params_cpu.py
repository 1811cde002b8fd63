"""No-GPU checks of `args.text_params` (the text encoder's parameters in a flat store of their own, stepped by FusedAdam in
the trunk's launch): the switch and its refusals, the text store's layout and the segment table of bpm_adam_step_sets
over both stores built from HOST tensors (ops._DRY_RUN: nothing is launched), and distributed.GradSync on gloo (world 2)
with a model stub that holds two flat stores."""
import ctypes as C
import os
import socket
import sys
from types import SimpleNamespace

import pytest
import torch
import torch.distributed as dist
import torch.multiprocessing as mp

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, engine, ops
from bpmult_amd.models import get_model
from bpmult_amd.models.bert import EMBED_PARAMS, LAYER_PARAMS
from bpmult_amd.models.bpmult import BertEncoder

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def _save_tiny(path):
    from transformers import BertConfig, BertModel
    torch.manual_seed(0)
    BertModel(BertConfig(vocab_size=60, hidden_size=32, num_hidden_layers=2, num_attention_heads=2, intermediate_size=64,
                         max_position_embeddings=32)).save_pretrained(path)
    return str(path)


def _args(**kw):
    a = dict(model="mmtrvat", orig_d_l=32, orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=40, vonly=True, lonly=True, aonly=True,
             num_heads=4, layers=1, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0., res_dropout=0.,
             out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6, bert_model="unused", text_features=True,
             num_vectors_l=48, num_vectors_a=48, num_vectors_v=48, precision="bf16")
    a.update(kw)
    return SimpleNamespace(**a)


@pytest.fixture
def dry_run():
    ops._DRY_RUN = True
    try:
        yield
    finally:
        ops._DRY_RUN = False


def test_switch_default_and_validation(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    assert BertEncoder(_args()).text_params == "torch"
    assert BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip")).text_params == "torch"
    assert BertEncoder(_args(bert_model=d, text_features=False, text_encoder="hip", text_params="flat")).text_params == "flat"
    for bad in ("FLAT", "hip", "", None):
        with pytest.raises(ValueError, match="text_params"):
            BertEncoder(_args(text_params=bad))
    with pytest.raises(ValueError, match="text_params='flat' needs text_encoder='hip'"):
        BertEncoder(_args(bert_model=d, text_features=False, text_params="flat"))
    with pytest.raises(ValueError, match="text_params='flat' needs text_encoder='hip'"):
        get_model(_args(bert_model=d, text_features=False, text_encoder="torch", text_params="flat"))


def test_names_and_state_dict_keys_are_unchanged(tmp_path):
    d = _save_tiny(tmp_path / "bert")
    m_t = get_model(_args(bert_model=d, text_features=False, text_encoder="hip"))
    m_f = get_model(_args(bert_model=d, text_features=False, text_encoder="hip", text_params="flat"))
    assert list(m_t.state_dict()) == list(m_f.state_dict())
    assert [n for n, _ in m_t.named_parameters()] == [n for n, _ in m_f.named_parameters()]


@pytest.mark.parametrize("embeddings", ["hip", "torch"])
def test_text_store_layout_and_the_table_over_both_stores(dry_run, tmp_path, embeddings):
    """Hidden-40 trunk (column and parameter padding) + the tiny text store: the store's layout, and the segment table of
    bpm_adam_step_sets over both."""
    d = _save_tiny(tmp_path / "bert")
    m = get_model(_args(bert_model=d, text_features=False, text_encoder="hip", text_embeddings=embeddings, text_params="flat"))
    before = {n: p.detach().clone() for n, p in m.named_parameters()}
    stores = m._flat_stores()
    assert len(stores) == 2 and stores[0] is m._ensure_store() and stores[1] is m.enc.flat_store()
    assert len(get_model(_args())._flat_stores()) == 1
    trunk, text = stores
    named = dict(m.named_parameters())
    # membership: the 16 parameters of every layer, the five embedding parameters only when they run on HIP; never the pooler
    want = [f"enc.bert.encoder.layer.{i}.{n}" for i in (1, 0) for n in LAYER_PARAMS]
    if embeddings == "hip":
        want += [f"enc.bert.embeddings.{n}" for n in EMBED_PARAMS]
    assert text.names == want                                                   # reverse execution order
    assert not any(n in trunk.params for n in text.names)
    for n in text.names:                                                        # views into the master, values kept
        assert named[n].data_ptr() == text.master.data_ptr() + 4 * text.off[n] and torch.equal(named[n], before[n]), n
    assert text.still_flat()
    secs = text.sections
    assert list(secs) == ["layer1", "layer0"] + (["embeddings"] if embeddings == "hip" else [])
    bounds = [secs[k] for k in secs]
    assert bounds[0][0] == 0 and bounds[-1][1] == text.total and all(a[1] == b[0] for a, b in zip(bounds, bounds[1:]))
    for i in (0, 1):
        lo, hi = secs[f"layer{i}"]
        assert all(lo <= text.off[n] < hi for n in text.names if f".layer.{i}." in n)
    # every weight shadow is a plain image: the optimizer kernel writes all of them, no second pack is left
    assert len(text._adam_plain) == 12 and text._rest_table is None
    ld = 32
    assert text._shadow_off["layer0.qkv#1"] == text._shadow_off["layer0.qkv"] + 32 * ld
    assert text._shadow_off["layer0.qkv#2"] == text._shadow_off["layer0.qkv"] + 64 * ld

    frozen = "enc.bert.encoder.layer.0.output.dense.weight"
    group_ofs = [{n: (1 if trunk.params[n].ndim <= 1 else 0) for n in trunk.names},
                 {n: (1 if text.params[n].ndim <= 1 else 0) for n in text.names if n != frozen}]
    tab, host, nseg, nblk = engine.adam_sets_table(stores, group_ofs)
    assert nseg == len(host) and tab.numel() == nseg * C.sizeof(_lib.AdamSeg)
    blk, seen = 0, [[], []]
    for sg in host:
        assert sg.blk0 == blk and sg.n4 > 0                                     # sorted by blk0, no gap
        blk += ops.adam_blocks(sg.n4)
        si, gi = (sg.group & 0xffffffff) >> _lib.ADAM_SET_SHIFT, sg.group & 0xff
        assert si in (0, 1) and gi in (0, 1, 0xff)                              # one set, one group (0xff: -1, not stepped)
        seen[si].append((4 * sg.off4, 4 * (sg.off4 + sg.n4), gi))
        if sg.dst:
            assert sg.cols % 4 == 0 and sg.rows * sg.cols <= 4 * sg.n4 and sg.dst_ld >= sg.cols
    assert blk == nblk
    for si, st in enumerate(stores):                                            # each store covered exactly once, in order
        assert seen[si][0][0] == 0 and seen[si][-1][1] == st.total
        assert all(a[1] == b[0] for a, b in zip(seen[si], seen[si][1:]))
        for n in st.names:
            a = st.off[n]
            (gi,) = [g for lo, hi, g in seen[si] if lo <= a < hi]
            assert gi == (group_ofs[si].get(n, -1) & 0xff), n
    assert [g for lo, hi, g in seen[1] if lo == text.off[frozen]] == [0xff]
    assert _lib.adam_set_group(1, -1) == (1 << 8) | 0xff and _lib.adam_set_group(0, 3) == 3


def test_entry_refuses_bad_arguments_before_any_launch(dry_run):
    """bpm_adam_step_sets reads the HOST copies of the table and the sets for every check: the refusals can be exercised
    without a device (a call that passed them would launch)."""
    _lib.build()
    L = _lib.lib()
    ERR_ARG, ERR_ALIGN = -1, -2
    assert L.bpm_error_string(ERR_ARG) and L.bpm_error_string(ERR_ALIGN)
    buf = [torch.zeros(4096 + 4) for _ in range(8)]
    al = lambda t: t[(-(t.data_ptr() // 4)) % 4:][:4096]                       # a 16-byte aligned window
    a, b = [al(t) for t in buf[:4]], [al(t) for t in buf[4:]]

    def call(segs, sets, groups=None, ngroups=None, nsets=None, table_host=True, scale_dev=None):
        _, sets_host, _ = ops.adam_sets(sets) if sets else (None, None, None)
        tab = (_lib.AdamSeg * len(segs))(*segs)
        groups = ops.adam_groups(groups or [dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=1)])
        return L.bpm_adam_step_sets(0, C.addressof(tab), tab if table_host else None, len(segs), sum(ops.adam_blocks(s.n4) for s in segs),
                                    C.addressof(sets_host) if sets else None, sets_host, len(sets or ()) if nsets is None else nsets, groups,
                                    len(groups) if ngroups is None else ngroups, 1.0, scale_dev, None, None, None, 0, None)

    def seg(si, gi, off4, n4, blk0):
        s = _lib.AdamSeg()
        s.off4, s.n4, s.blk0, s.group = off4, n4, blk0, _lib.adam_set_group(si, gi)
        return s

    good = [seg(0, 0, 0, 1024, 0), seg(1, -1, 0, 1024, 1)]
    assert call(good, [a, b], table_host=False) == ERR_ARG                     # NULL host table
    assert call(good, None) == ERR_ARG                                          # NULL sets
    assert call(good, [a, b], nsets=0) == ERR_ARG and call(good, [a, b], nsets=5) == ERR_ARG
    assert call(good, [a]) == ERR_ARG                                           # a segment in set 1 of one set
    assert call(good, [a, b], ngroups=0) == ERR_ARG and call(good, [a, b], ngroups=17) == ERR_ARG
    assert call(good, [a, b], groups=[dict(lr=1e-3, betas=(0.9, 0.999), eps=1e-8, weight_decay=0.0, step=0)]) == ERR_ARG
    assert call([seg(0, 0, 0, 1024, 0), seg(1, 0, 1, 1024, 1)], [a, b]) == ERR_ARG        # reaches beyond its set
    assert call([seg(0, 0, 0, 1024, 0), seg(1, 0, 0, 1024, 2)], [a, b]) == ERR_ARG        # a gap in the blocks
    odd = [t[1:] for t in a]                                                    # 4-byte aligned only
    assert call([seg(0, 0, 0, 1023, 0)], [[t[:4092] for t in odd]]) == ERR_ALIGN
    assert call(good, [a, b], scale_dev=a[0].data_ptr() + 2) == ERR_ALIGN
    with pytest.raises(ValueError, match="buffer sets"):
        ops.adam_sets([a] * 5)


# ---------------------------------------------------------------------------------------------------------------------
# GradSync over two stores (gloo, host tensors)
# ---------------------------------------------------------------------------------------------------------------------
def _free_port():
    s = socket.socket()
    s.bind(("127.0.0.1", 0))
    p = s.getsockname()[1]
    s.close()
    return p


class _Store:
    """What GradSync needs of engine.ParamStore: the flat gradient buffer, the names it owns, its sections."""

    def __init__(self, sizes, prefix=""):
        self.off, off = {}, 0
        for n, k in sizes.items():
            self.off[n] = off
            off += k
        self.total = off
        self.gflat = torch.zeros(off)
        self.params = {prefix + n: torch.nn.Parameter(torch.zeros(k)) for n, k in sizes.items()}     # the model's names
        for (n, k), p in zip(sizes.items(), self.params.values()):
            p.grad = self.gflat[self.off[n]: self.off[n] + k]
        self.sections = {n: (self.off[n], self.off[n] + sizes[n]) for n in sizes}


TRUNK = {"fuse": 300, "level2.layer0": 1000, "level1.layer0": 700, "proj": 130}
TEXT = {"layer1": 900, "layer0": 900, "embeddings": 2100}


class _Model(torch.nn.Module):
    def __init__(self):
        super().__init__()
        self._store, self._text = _Store(TRUNK), _Store(TEXT, "enc.")
        self.pooler = torch.nn.Parameter(torch.zeros(6))
        self.head = torch.nn.Parameter(torch.zeros(2))
        self._grad_ready_hook = None
        self.reported = []

    def _flat_stores(self):
        return [self._store, self._text]

    def named_parameters(self, *a, **k):
        yield from self._store.params.items()
        yield from self._text.params.items()
        yield "enc.bert.pooler", self.pooler
        yield "head", self.head

    def backward(self, trunk, text, tail):
        """The order of a real step: the trunk's sections in reverse execution order, then the text encoder's -- layer
        n-1 ... 0, then the embeddings -- each reported when its slice is final."""
        for st, contrib, names in ((self._store, trunk, TRUNK), (self._text, text, TEXT)):
            for n in names:
                lo, hi = st.sections[n]
                st.gflat[lo:hi] += contrib[lo:hi]
                if self._grad_ready_hook is not None:
                    self.reported.append((st is self._text, n))
                    self._grad_ready_hook(st.gflat, lo, hi, None)
        for p, g in ((self.pooler, tail[:6]), (self.head, tail[6:])):
            p.grad = g.clone() if p.grad is None else p.grad + g


def _worker(rank, world, port, out):
    sys.path.insert(0, ROOT)
    os.environ["MASTER_ADDR"], os.environ["MASTER_PORT"] = "127.0.0.1", str(port)
    dist.init_process_group("gloo", rank=rank, world_size=world)
    import bpmult_amd.distributed as D
    nt, nx = sum(TRUNK.values()), sum(TEXT.values())
    gen = lambda r, step: torch.randn(nt + nx + 8, generator=torch.Generator().manual_seed(100 * r + step))
    res = {}
    for mode in ("plain", "optimizer", "auto_sum"):
        model = _Model()
        opt = SimpleNamespace(pending_grad_scale=None) if mode == "optimizer" else None
        # "auto" resolves on BOTH buffers' bytes: the threshold lies above either buffer alone and below their sum
        D.AUTO_BF16_BYTES = 4 * (nt + nx) - 4 if mode == "auto_sum" else 1 << 30
        assert 4 * max(nt, nx) < 4 * (nt + nx) - 4
        sync = D.GradSync(model, bucket_bytes=4 * 256, optimizer=opt, compress="auto" if mode == "auto_sum" else "none")
        seen = []
        real = sync._exchange

        def spy(flat, lo, hi, real=real, seen=seen, model=model):
            seen.append((flat is model._text.gflat, lo, hi))
            real(flat, lo, hi)
        sync._exchange = spy
        for step, active in ((0, False), (1, True)):
            sync.active = active
            v = gen(rank, step)
            model.backward(v[:nt], v[nt:nt + nx], v[nt + nx:])
            flattened = []
            orig = torch._utils._flatten_dense_tensors
            torch._utils._flatten_dense_tensors = lambda ts: (flattened.append([t.numel() for t in ts]), orig(ts))[1]
            try:
                sync.finish()
            finally:
                torch._utils._flatten_dense_tensors = orig
            if not active:                                  # a micro-step that is not the last one exchanges nothing
                assert not seen and not sync.handles and not flattened
                assert torch.equal(torch.cat([model._store.gflat, model._text.gflat]), v[:nt + nx])
            else:
                assert flattened == [[6, 2]], flattened      # the tail list: what is in no store, and nothing else
        # the text sections arrive layer n-1 ... 0, then the embeddings, after the trunk's
        assert [n for is_text, n in model.reported if is_text][-3:] == ["layer1", "layer0", "embeddings"]
        assert [s for s in seen if s[0]] == [(True,) + model._text.sections[n] for n in TEXT]
        cover = torch.zeros(nt + nx)
        for is_text, lo, hi in seen:                        # every element of both buffers exchanged exactly once
            cover[(nt if is_text else 0) + lo: (nt if is_text else 0) + hi] += 1
        assert bool((cover == 1).all())
        want = sum(gen(r, 0) + gen(r, 1) for r in range(world))
        scale = 1.0 if mode == "optimizer" else 1.0 / world
        got = torch.cat([model._store.gflat, model._text.gflat, model.pooler.grad, model.head.grad])
        res[mode] = float((got - want * scale).abs().max() / want.abs().max())
        if mode == "optimizer":
            assert opt.pending_grad_scale == 1.0 / world    # the buffers keep the SUM; the optimizer's kernel scales
        if mode == "auto_sum":
            assert sync.compress == "bf16"
        else:
            assert sync.compress == "none"
    out[rank] = res
    dist.destroy_process_group()


def test_gradsync_exchanges_both_stores_in_place():
    world = 2
    port = _free_port()
    out = mp.Manager().dict()
    mp.spawn(_worker, args=(world, port, out), nprocs=world, join=True)
    assert len(out) == world
    for r, e in out.items():
        assert e["plain"] < 1e-6 and e["optimizer"] < 1e-6, (r, e)
        assert e["auto_sum"] < 2e-2, (r, e)                 # bf16 slices: the bound of test_gradsync_gloo_cpu.py
