"""No-GPU checks of the per-sample attention entries (bpm_attn_*_bmask / *_kbmask, bpm_attn_bwd_dbias_bmask), in the style
of tests/attn_cases.py: calls at made-up aligned addresses against the -DBPM_LAB build in dry mode (nothing is launched,
nothing is dereferenced).
  * the ABI: every new export is bound, the structs mirror the header;
  * the argument rules: every BPM_ERR_ARG case of the header comment, per entry;
  * dispatch: at batch stride 0 each entry makes the launches of its *_hmask / *_kamask sibling (the per-sample kernel of
    the same compute type and head_dim on the same grid), with non-zero strides the same grid; the tile count and workspace
    of the per-sample bias gradient are what its shapes imply;
  * ops: the 8-tuple form of attn_amasks and the 4-tuple form of attn_dbias."""
import ctypes as C
import re

import pytest
import torch

import bpmult_amd  # noqa: F401
from bpmult_amd import _lib, ops
from bpmult_amd._lib import BPM_BF16 as BF, BPM_F32 as F32

import attn_cases as AC
from rowops_cases import BASE, Addr, run

ERR_ARG = -1
B, H, T, S = 3, 2, 65, 129
LDM, LDT = 132, 68                        # up4(S), up4(T)
ENTRIES = ("fwd", "bwd_dq", "bwd_dkv", "maps", "head_maps")


@pytest.fixture(scope="module")
def lab():
    _lib.build_lab()
    with _lib.lab_library() as L:
        yield L


def problems(entry, dhp=64, n=1):
    if entry == "head_maps":
        A = Addr()
        q = (_lib.AttnHeadMapProblem * n)()
        for p in q:
            p.B, p.H, p.T, p.S, p.dh, p.dhp, p.mask_off, p.q_stride = B, H, T, S, dhp, dhp, 0, 1
            p.Q, p.K, p.lse, p.W, p.ldw = A(), A(), A(), A(), S
            p.head_stride, p.batch_stride = T * S, H * T * S
        return q
    return AC.problems(n, B=B, H=H, T=T, S=S, dhp=dhp, maps=entry == "maps")


def images(n=1, per_head=True, per_sample=True, cls=None):
    A = Addr()
    A.next = BASE + (1 << 40)
    m = ((cls or _lib.AttnBMask) * n)()
    for a in m:
        a.mask, a.ldm, a.maskT, a.ldt = A(), LDM, A(), LDT
        if per_head:
            a.head_stride, a.head_strideT = T * LDM, S * LDT
        if per_sample and cls is None:
            a.batch_stride, a.batch_strideT = (H if per_head else 1) * T * LDM, (H if per_head else 1) * S * LDT
    return m


def call(L, entry, fam="bmask", dt=BF, dhp=64, n=1, edit=None, edit_p=None, per_head=True, per_sample=True, masks="auto", kmasks="auto"):
    """bpm_attn_<entry>_<fam>: fam bmask / kbmask, or hmask / kamask (the siblings, with bpm_attn_hmask)"""
    q = problems(entry, dhp, n)
    m = images(n, per_head, per_sample, _lib.AttnHMask if fam in ("hmask", "kamask") else None)
    k = AC.masks_for("kmask", q)
    if edit:
        for key, v in edit.items():
            setattr(m[0], key, v)
    if edit_p:
        for key, v in edit_p.items():
            setattr(q[0], key, v)
    args = [dt, q]
    if fam.startswith("k"):
        args.append(k if kmasks == "auto" else kmasks)
    args.append(m if masks == "auto" else masks)
    args += [n, None] if "maps" in entry else [n, 5, None]
    return getattr(L, f"bpm_attn_{entry}_{fam}")(*args)


def dbias(L, dt=BF, dhp=64, edit=None, edit_o=None, edit_p=None, form=(1, 1), per_sample_mask=True, with_k=False, query=False, ws="fits",
          Bn=B, Hn=H, Tn=T, Sn=S):
    q = AC.problems(1, B=Bn, H=Hn, T=Tn, S=Sn, dhp=dhp)
    ldm = AC.up4(Sn)
    m = (_lib.AttnBMask * 1)()
    A = Addr()
    A.next = BASE + (1 << 40)
    m[0].mask, m[0].ldm, m[0].maskT, m[0].ldt = A(), ldm, A(), AC.up4(Tn)
    m[0].head_stride, m[0].head_strideT = Tn * ldm, Sn * AC.up4(Tn)
    if per_sample_mask:
        m[0].batch_stride, m[0].batch_strideT = Hn * Tn * ldm, Hn * Sn * AC.up4(Tn)
    o = (_lib.AttnDBiasB * 1)()
    o[0].dB, o[0].lddb = A(), ldm
    o[0].head_stride = Tn * ldm if form[1] > 1 else 0
    o[0].batch_stride = (Hn if form[1] > 1 else 1) * Tn * ldm if form[0] > 1 else 0
    for target, ed in ((m, edit), (o, edit_o), (q, edit_p)):
        for key, v in (ed or {}).items():
            setattr(target[0], key, v)
    need = L.bpm_attn_bwd_dbias_bmask_ws_bytes(q, o, 1)
    if query:
        return need
    wsp = {"none": None, "misaligned": BASE - (1 << 30) + 8}.get(ws, BASE - (1 << 30))
    k = AC.masks_for("kmask", q) if with_k else None
    return L.bpm_attn_bwd_dbias_bmask(dt, q, m, k, o, 1, 5, wsp, need - 16 if ws == "short" else need, None)


# ---------------------------------------------------------------------------------------------------------------------
# ABI
# ---------------------------------------------------------------------------------------------------------------------
NEW = [f"bpm_attn_{e}_{f}" for f in ("bmask", "kbmask") for e in ENTRIES] + ["bpm_attn_bwd_dbias_bmask", "bpm_attn_bwd_dbias_bmask_ws_bytes"]


def test_every_new_export_is_declared_bound_and_exported(lab):
    header = open(AC.__file__.replace("tests/attn_cases.py", "include/bpmult_hip.h")).read()
    declared = set(re.findall(r"^\s*(?:int|size_t)\s+(bpm_\w+)\s*\(", header, flags=re.M))
    _lib.build()
    product = _lib.lib()
    for name in NEW:
        assert name in declared and name in _lib.SIGNATURES, name
        assert hasattr(product, name) and hasattr(lab, name), name
    assert "Per-sample masks do not exist" not in header
    for cname, cls in (("bpm_attn_bmask", _lib.AttnBMask), ("bpm_attn_dbias_b", _lib.AttnDBiasB)):
        body = re.search(r"typedef struct %s \{(.*?)\} %s;" % (cname, cname), header, flags=re.S).group(1)
        body = re.sub(r"/\*.*?\*/", "", body, flags=re.S)
        names = [n.strip().lstrip("*") for decl in body.split(";") if decl.strip()
                 for n in [decl.strip().split(",")[0].split()[-1]] + decl.strip().split(",")[1:]]
        assert names == [f[0] for f in cls._fields_], (cname, names)
    assert C.sizeof(_lib.AttnBMask) == 64 and C.sizeof(_lib.AttnDBiasB) == 32
    assert _lib.SIGNATURES["bpm_attn_fwd_hmask"][2] == C.POINTER(_lib.AttnHMask), "the existing entries keep their structs"


# ---------------------------------------------------------------------------------------------------------------------
# argument rules
# ---------------------------------------------------------------------------------------------------------------------
IMG, IMGT = T * LDM, S * LDT
STRIDE_FAULTS = {
    "batch stride not a multiple of 4": dict(batch_stride=H * IMG + 2),
    "batch stride below H head strides": dict(batch_stride=H * IMG - 4),
    "batch stride 2^31": dict(batch_stride=1 << 31),
    "negative batch stride": dict(batch_stride=-4),
}
STRIDE_FAULTS_T = {
    "batch strideT not a multiple of 4": dict(batch_strideT=H * IMGT + 2),
    "batch strideT below H head strides": dict(batch_strideT=H * IMGT - 4),
    "batch strideT 2^31": dict(batch_strideT=1 << 31),
}
SIBLING_FAULTS = {
    "null mask": dict(mask=None), "ldm < S": dict(ldm=128), "ldm not a multiple of 4": dict(ldm=134), "mask 8 bytes off": dict(mask=BASE + (1 << 42) + 8),
    "head stride short": dict(head_stride=IMG - 4), "head stride not a multiple of 4": dict(head_stride=IMG + 2), "head stride 2^31": dict(head_stride=1 << 31),
}
SIBLING_FAULTS_T = {"null maskT": dict(maskT=None), "ldt < T": dict(ldt=64), "maskT 4 bytes off": dict(maskT=BASE + (1 << 42) + 4),
                    "head strideT short": dict(head_strideT=IMGT - 4)}


def reads_transpose(entry):
    return entry in ("bwd_dkv", "maps", "head_maps")


@pytest.mark.parametrize("fam", ["bmask", "kbmask"])
@pytest.mark.parametrize("entry", ENTRIES)
def test_argument_rules_of_the_mask_entries(lab, fam, entry):
    ok = run(lab, lambda L: call(L, entry, fam))
    assert ok["rc"] == 0 and len(ok["launches"]) == 1, ok
    for name, f in {**STRIDE_FAULTS, **SIBLING_FAULTS}.items():
        r = run(lab, lambda L: call(L, entry, fam, edit=f))
        assert r == {"rc": ERR_ARG, "launches": []}, (name, r)
    for name, f in {**STRIDE_FAULTS_T, **SIBLING_FAULTS_T}.items():
        r = run(lab, lambda L: call(L, entry, fam, edit=f))
        if reads_transpose(entry):
            assert r == {"rc": ERR_ARG, "launches": []}, (name, r)
        else:
            assert r["rc"] == 0, (name, "the forward and dQ entries do not read the transpose", r)
    # one image per sample without a head stride: the sample stride must cover one image
    assert run(lab, lambda L: call(L, entry, fam, per_head=False))["rc"] == 0
    assert run(lab, lambda L: call(L, entry, fam, per_head=False, edit=dict(batch_stride=IMG - 4)))["rc"] == ERR_ARG
    assert run(lab, lambda L: call(L, entry, fam, per_head=False, edit=dict(batch_stride=IMG, batch_strideT=IMGT)))["rc"] == 0
    # the largest legal stride, no mask array, no key-mask array, a dtype that is neither, no instantiation
    assert run(lab, lambda L: call(L, entry, fam, edit=dict(batch_stride=(1 << 31) - 4)))["rc"] == 0
    assert run(lab, lambda L: call(L, entry, fam, masks=None))["rc"] == ERR_ARG
    if fam == "kbmask":
        assert run(lab, lambda L: call(L, entry, fam, kmasks=None))["rc"] == ERR_ARG
    assert run(lab, lambda L: call(L, entry, fam, dt=7))["rc"] == ERR_ARG
    assert run(lab, lambda L: call(L, entry, fam, dhp=48))["rc"] == ERR_ARG
    assert run(lab, lambda L: call(L, entry, fam, n=_lib.MAX_GROUP))["rc"] == 0
    assert run(lab, lambda L: call(L, entry, fam, n=_lib.MAX_GROUP + 1))["rc"] == ERR_ARG
    assert run(lab, lambda L: call(L, entry, fam, edit_p=dict(T=0)))["rc"] == ERR_ARG
    if "maps" not in entry:
        r = run(lab, lambda L: call(L, entry, fam, edit_p=dict(dS=BASE + (1 << 42), Pd=BASE + (1 << 43), xs_q=LDM, xs_h=IMG, xs_b=H * IMG, S=128)))
        assert r == {"rc": ERR_ARG, "launches": []}, ("dS / Pd set", r)


def test_argument_rules_of_the_bias_gradient(lab):
    for form in ((1, 1), (1, H), (B, 1), (B, H)):
        for with_k in (False, True):
            r = run(lab, lambda L: dbias(L, form=form, with_k=with_k))
            assert r["rc"] == 0 and len(r["launches"]) >= 1, (form, r)
    faults = {
        "output batch stride not a multiple of 4": dict(edit_o=dict(batch_stride=H * IMG + 2), form=(B, H)),
        "output batch stride below H head strides": dict(edit_o=dict(batch_stride=H * IMG - 4), form=(B, H)),
        "output batch stride below one image": dict(edit_o=dict(batch_stride=IMG - 4), form=(B, 1)),
        "output batch stride 2^31": dict(edit_o=dict(batch_stride=1 << 31), form=(B, H)),
        "null dB": dict(edit_o=dict(dB=None)), "lddb < S": dict(edit_o=dict(lddb=128)), "lddb not a multiple of 4": dict(edit_o=dict(lddb=131)),
        "dB 8 bytes off": dict(edit_o=dict(dB=BASE + (1 << 42) + 8)), "output head stride short": dict(edit_o=dict(head_stride=IMG - 4), form=(1, H)),
        "dS / Pd set": dict(edit_p=dict(dS=BASE + (1 << 42), Pd=BASE + (1 << 43))), "T = 0": dict(edit_p=dict(T=0)), "no lse": dict(edit_p=dict(lse=None)),
        "workspace none": dict(ws="none", Hn=8, Tn=5, Sn=5, form=(B, 1)), "workspace short": dict(ws="short", Hn=8, Tn=5, Sn=5, form=(B, 1)),
        "workspace misaligned": dict(ws="misaligned", Hn=8, Tn=5, Sn=5, form=(B, 1)),
        **{"mask: " + k: dict(edit=v) for k, v in {**STRIDE_FAULTS, **SIBLING_FAULTS}.items()},
    }
    for name, kw in faults.items():
        r = run(lab, lambda L: dbias(L, **kw))
        assert r == {"rc": ERR_ARG, "launches": []}, (name, r)
    assert run(lab, lambda L: dbias(L, dt=7))["rc"] == ERR_ARG
    assert run(lab, lambda L: dbias(L, dhp=48))["rc"] == ERR_ARG
    assert run(lab, lambda L: dbias(L, dhp=48, query=True))["rc"] == 0, "a refused call needs no workspace"
    # the transposed image is not read
    assert run(lab, lambda L: dbias(L, edit=dict(maskT=None, batch_strideT=2)))["rc"] == 0


# ---------------------------------------------------------------------------------------------------------------------
# dispatch
# ---------------------------------------------------------------------------------------------------------------------
def as_sibling(kernel):
    k = kernel.replace("attn_bmask_kernel", "attn_amask_kernel").replace("attn_kbmask_kernel", "attn_kamask_kernel")
    k = k.replace("AGroupKB", "AGroupKA").replace("AGroupB", "AGroupA")
    return k


@pytest.mark.parametrize("dt", [BF, F32])
@pytest.mark.parametrize("dhp", [32, 64, 128, 256])
@pytest.mark.parametrize("fam,sib", [("bmask", "hmask"), ("kbmask", "kamask")])
def test_stride_zero_makes_the_launches_of_the_sibling(lab, dt, dhp, fam, sib):
    for entry in ENTRIES:
        old = run(lab, lambda L: call(L, entry, sib, dt, dhp))
        for per_sample in (False, True):
            new = run(lab, lambda L: call(L, entry, fam, dt, dhp, per_sample=per_sample))
            assert new["rc"] == old["rc"] == 0 and len(new["launches"]) == len(old["launches"]) == 1
            (kn, gn, bn, _), (ko, go, bo, _) = new["launches"][0], old["launches"][0]
            assert (gn, bn) == (go, bo), (entry, "the same grid and block", new, old)
            assert "bmask_kernel" in kn and "bmask" not in ko, (kn, ko)
            if "maps" in entry:         # the same kernel family, and (where the note spells them) compute type and head_dim
                assert kn.replace("_bmask", "").split("<")[0] == ko.split("<")[0], (kn, ko)
                if "<" in kn and "<" in ko:
                    assert kn.split("<")[1].rstrip(">").split(",")[:2] == ko.split("<")[1].rstrip(">").split(",")[:2], (kn, ko)
            else:
                assert as_sibling(kn) == ko, (kn, ko)


def test_bias_gradient_tiles_and_workspace(lab):
    """T = 65, S = 129: 2 x 3 tiles per image; B = 3, H = 2.  Images x terms: [T,S] 1 x 6, [H,T,S] 2 x 3, [B,1,T,S] 3 x 2,
    [B,H,T,S] 6 x 1.  The target is 768 workgroups at head_dim 64 and a split keeps at least 4 terms: only the shared form
    splits (2 workgroups of 3 terms), and its workspace is 2 x 65 x 132 floats -- what bpm_attn_bwd_dbias makes of it."""
    for form, (nimg, nsplit) in {(1, 1): (1, 2), (1, H): (2, 1), (B, 1): (3, 1), (B, H): (6, 1)}.items():
        r = run(lab, lambda L: dbias(L, form=form))
        need = run(lab, lambda L: dbias(L, form=form, query=True))["rc"]
        assert need == (nsplit * nimg * T * LDM * 4 if nsplit > 1 else 0), (form, need)
        assert r["rc"] == 0 and len(r["launches"]) == (2 if nsplit > 1 else 1), r
        assert "attn_dbias_bmask_kernel" in r["launches"][0][0] and r["launches"][0][1:3] == [nimg * nsplit * 6, 256], r
        if nsplit > 1:
            assert "attn_dbias_sum_bmask_kernel" in r["launches"][1][0], r
    # the forms bpm_attn_bwd_dbias has: the same grids and the same workspace
    for out_heads, form in (((), (1, 1)), ((0,), (1, H))):
        old = run(lab, lambda L: AC.dbias(L, B=B, H=H, T=T, S=S, per_head=(0,), out_heads=out_heads))
        new = run(lab, lambda L: dbias(L, form=form, per_sample_mask=False))
        assert [l[1:3] for l in old["launches"]] == [l[1:3] for l in new["launches"]], (old, new)
        assert run(lab, lambda L: AC.dbias(L, B=B, H=H, T=T, S=S, out_heads=out_heads, query=True)) == \
            run(lab, lambda L: dbias(L, form=form, query=True))
    # 8 heads, T = S = 5, result [B,1,T,S]: one tile per image, the 8 terms over two workgroups
    r = run(lab, lambda L: dbias(L, form=(B, 1), Hn=8, Tn=5, Sn=5))
    assert r["rc"] == 0 and [l[1] for l in r["launches"]] == [B * 2, 1], r
    assert run(lab, lambda L: dbias(L, form=(B, 1), Hn=8, Tn=5, Sn=5, query=True))["rc"] == 2 * B * 5 * 8 * 4


# ---------------------------------------------------------------------------------------------------------------------
# ops
# ---------------------------------------------------------------------------------------------------------------------
def test_ops_tuple_forms():
    a = ops.attn_amasks([(BASE, 8, BASE + 4096, 8, 64, 64, 128, 128)])
    assert a._type_ is _lib.AttnBMask and (a[0].head_stride, a[0].batch_stride, a[0].batch_strideT) == (64, 128, 128)
    assert ops.attn_amasks([(BASE, 8, BASE + 4096, 8, 64, 64)])._type_ is _lib.AttnHMask
    assert ops.attn_amasks([(BASE, 8, BASE + 4096, 8)])._type_ is _lib.AttnHMask
    mixed = ops.attn_amasks([(BASE, 8, BASE + 4096, 8), (BASE, 8, BASE + 4096, 8, 0, 0, 64, 64)])
    assert mixed._type_ is _lib.AttnBMask and mixed[0].batch_stride == 0 and mixed[1].batch_stride == 64
    o = ops.attn_dbias([(BASE, 8, 64, 128)])
    assert o._type_ is _lib.AttnDBiasB and (o[0].head_stride, o[0].batch_stride) == (64, 128)
    assert ops.attn_dbias([(BASE, 8, 64)])._type_ is _lib.AttnDBias
    assert ops._mask_entry("bpm_attn_fwd_hmask", a) == "bpm_attn_fwd_bmask"
    assert ops._mask_entry("bpm_attn_head_maps_kamask", a) == "bpm_attn_head_maps_kbmask"
    assert ops._mask_entry("bpm_attn_fwd_hmask", ops.attn_amasks([(BASE, 8, BASE + 4096, 8)])) == "bpm_attn_fwd_hmask"
