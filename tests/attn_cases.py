"""The case table of tests/test_attn_dispatch_cpu.py: calls of the attention entry points (csrc/attention.hip,
attn_maps.hip, attn_dbias.hip) at made-up aligned addresses.  The runner is rowops_cases.run: a -DBPM_LAB build in dry mode
(bpm_debug_rows_dry, which covers the attention launches too) says which launches each call makes; nothing is launched,
nothing is dereferenced.  `tools/rowops_dispatch.py --cases attn` runs the table against any lab build and writes the
record the test compares with (profiles/attn_dispatch.json, recorded from the tree that still had everything in the one
csrc/attention.hip).

A case is name -> function(L) -> return code of the entry (the byte count for bpm_attn_bwd_dbias_ws_bytes).  Its record is
{"rc": code, "launches": [[kernel, grid, block, 0], ...]}."""
import ctypes as C

from bpmult_amd import _lib
from bpmult_amd._lib import BPM_BF16 as BF, MAX_GROUP

from rowops_cases import BASE, DT, Addr, normalise, run  # noqa: F401  (run / normalise: the runner of both tables)

CASES = {}


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


def run_all(L):
    return {name: run(L, fn) for name, fn in CASES.items()}


PLAIN = ("fwd", "bwd", "bwd_dq", "bwd_dkv")
MASKED = tuple(f"{k}_{m}" for m in ("kmask", "amask", "hmask") for k in ("fwd", "bwd_dq", "bwd_dkv"))
MAPS = ("maps", "maps_amask", "maps_hmask")
DHPS = (32, 64, 128, 256)


def up4(x):
    return (x + 3) // 4 * 4


def shapes_of(n, T, S):
    """n (T, S) pairs: the given pair, or a list of pairs cycled"""
    pairs = T if isinstance(T, (list, tuple)) else [(T, S)]
    return [pairs[i % len(pairs)] for i in range(n)]


def problems(n=1, B=2, H=3, T=65, S=129, dh=None, dhp=64, xp=(), maps=False):
    """n problems with every pointer set; xp: indices of the problems that ask for dS / Pd"""
    A = Addr()
    q = ((_lib.AttnMapProblem if maps else _lib.AttnProblem) * max(n, 1))()
    for i, (p, (t, s)) in enumerate(zip(q, shapes_of(max(n, 1), T, S))):
        p.B, p.H, p.T, p.S, p.dh, p.dhp = B, H, t, s, dhp if dh is None else dh, dhp
        p.mask_off, p.q_pos0, p.q_stride = 1 + abs(s - t), 0, 1
        p.Q, p.K, p.lse = A(), A(), A()
        if maps:
            p.W, p.ldw = A(), s
            continue
        p.V, p.O, p.dO, p.delta, p.dQ, p.dK, p.dV = A(), A(), A(), A(), A(), A(), A()
        p.ldo = p.lddq = p.lddk = p.lddv = H * p.dh
        p.dq_scale, p.drop_p, p.drop_site = 0.125, 0.1, i
        if i in xp:
            p.dS, p.Pd, p.xs_q, p.xs_h, p.xs_b = A(), A(), up4(s), t * up4(s), H * t * up4(s)
    return q


def masks_for(kind, q, per_head=()):
    """the mask array of a *_kmask / *_amask / *_hmask entry for problems q; per_head: indices with one image per head"""
    A = Addr()
    A.next = BASE + (1 << 40)
    if kind == "kmask":
        m = (_lib.AttnKMask * len(q))()
        for a, p in zip(m, q):
            a.mask, a.ldm = A(), p.S
        return m
    m = ((_lib.AttnAMask if kind == "amask" else _lib.AttnHMask) * len(q))()
    for i, (a, p) in enumerate(zip(m, q)):
        a.mask, a.ldm, a.maskT, a.ldt = A(), up4(p.S), A(), up4(p.T)
        if i in per_head:
            a.head_stride, a.head_strideT = p.T * a.ldm, p.S * a.ldt
    return m


def kind_of(entry):
    return entry.rsplit("_", 1)[-1] if entry.endswith("mask") else None


def attn(L, entry, dt=BF, n=1, edit=None, per_head=(), masks="auto", pair=7, probs="auto", **kw):
    """one call of bpm_attn_<entry>; edit(q, m) changes the problems / masks before the call"""
    maps = entry.startswith("maps")
    q = problems(n, maps=maps, **kw)
    kind = kind_of(entry)
    m = masks_for(kind, q, per_head) if kind else None
    if edit:
        edit(q, m)
    args = [dt, q if probs == "auto" else probs]
    if kind:
        args.append(m if masks == "auto" else masks)
    args += [n, None] if maps else [n, 5, None]
    L.bpm_debug_attn_pair(pair)
    try:
        return getattr(L, "bpm_attn_" + entry)(*args)
    finally:
        L.bpm_debug_attn_pair(7)


def dbias(L, dt=BF, n=1, edit=None, per_head=(), out_heads=(), ws="fits", query=False, outs="auto", masks="auto", **kw):
    """bpm_attn_bwd_dbias with the workspace bpm_attn_bwd_dbias_ws_bytes asks for (query: return that size instead);
    out_heads: indices of the problems whose dB has one image per head"""
    q = problems(n, **kw)
    m = masks_for("hmask", q, per_head)
    o = (_lib.AttnDBias * max(n, 1))()
    A = Addr()
    A.next = BASE + (1 << 41)
    for i, (d, p) in enumerate(zip(o, q)):
        d.dB, d.lddb = A(), up4(p.S)
        if i in out_heads:
            d.head_stride = p.T * d.lddb
    if edit:
        edit(q, m, o)
    o = o if outs == "auto" else outs
    need = L.bpm_attn_bwd_dbias_ws_bytes(q, o, n)
    if query:
        return need
    wsp = {"none": None, "misaligned": BASE - (1 << 30) + 8}.get(ws, BASE - (1 << 30))
    return L.bpm_attn_bwd_dbias(dt, q, m if masks == "auto" else masks, o, n, 5, wsp, need - 16 if ws == "short" else need, None)


def setp(i, **fields):
    """edit: set fields of problem i"""
    def f(q, *_):
        for k, v in fields.items():
            setattr(q[i], k, v)
    return f


def setm(i, **fields):
    """edit: set fields of mask i"""
    def f(q, m, *_):
        for k, v in fields.items():
            setattr(m[i], k, v)
    return f


def seto(i, **fields):
    """edit: set fields of bias-gradient output i"""
    def f(q, m, o):
        for k, v in fields.items():
            setattr(o[i], k, v)
    return f


def both(*edits):
    def f(*a):
        for e in edits:
            e(*a)
    return f


# ---------------------------------------------------------------------------------------------------------------------
# every entry x dtype x padded head_dim (48: no instantiation), and a dtype that is neither
# ---------------------------------------------------------------------------------------------------------------------
for _dn, _dt in list(DT.items()) + [("dtype 7", 7)]:
    for _d in (DHPS + (48,)) if _dt != 7 else (64,):
        for _e in PLAIN + MASKED + MAPS:
            case(f"{_e} {_dn} dhp={_d}")(lambda L, e=_e, dt=_dt, d=_d: attn(L, e, dt, dhp=d))
        case(f"bwd_dbias {_dn} dhp={_d}")(lambda L, dt=_dt, d=_d: dbias(L, dt, dhp=d))
        case(f"bwd_dbias per head {_dn} dhp={_d}")(lambda L, dt=_dt, d=_d: dbias(L, dt, dhp=d, per_head=(0,), out_heads=(0,)))
        case(f"bwd_dq with dS / Pd {_dn} dhp={_d}")(lambda L, dt=_dt, d=_d: attn(L, "bwd_dq", dt, dhp=d, S=128, xp=(0,)))
        case(f"maps_hmask per head {_dn} dhp={_d}")(lambda L, dt=_dt, d=_d: attn(L, "maps_hmask", dt, dhp=d, per_head=(0,)))
    case(f"fwd {_dn} dh=25 dhp=32")(lambda L, dt=_dt: attn(L, "fwd", dt, dh=25, dhp=32))
for _d in DHPS + (48,):
    case(f"bwd_dbias_ws_bytes dhp={_d}")(lambda L, d=_d: dbias(L, dhp=d, query=True))

# ---------------------------------------------------------------------------------------------------------------------
# block pairing (bpm_debug_attn_pair 0 / 7; 2 and 5: one kernel without the other): odd and even block counts, a single
# block, T != S (the dK / dV grid runs over S, the others' over T)
# ---------------------------------------------------------------------------------------------------------------------
SIZES = (1, 63, 64, 65, 129)
for _pair in (0, 7):
    for _bh in (1, 6):
        for _T in SIZES:
            for _S in SIZES:
                for _e in ("fwd", "bwd") if _S == 64 else ("bwd",):        # the forward grid does not depend on S
                    case(f"{_e} pair={_pair} B*H={_bh} T={_T} S={_S}")(
                        lambda L, e=_e, pr=_pair, bh=_bh, T=_T, S=_S: attn(L, e, pair=pr, B=1, H=bh, T=T, S=S))
        for _T, _S in ((63, 129), (129, 64)) if _bh == 6 else ():
            for _e in ("bwd_dq", "bwd_dkv") + MASKED:
                case(f"{_e} pair={_pair} B*H={_bh} T={_T} S={_S}")(
                    lambda L, e=_e, pr=_pair, bh=_bh, T=_T, S=_S: attn(L, e, pair=pr, B=bh, H=1, T=T, S=S))
for _pair in (2, 5):
    for _e in ("fwd", "bwd", "bwd_dq_kmask", "bwd_dkv_amask"):
        case(f"{_e} pair={_pair} T=129 S=257 x 2")(lambda L, e=_e, pr=_pair: attn(L, e, pair=pr, n=2, T=129, S=257))

# ---------------------------------------------------------------------------------------------------------------------
# the dQ pass with dS / Pd (XP): asked for by some problems of a group and not by others, parts 1, 2, 3
# ---------------------------------------------------------------------------------------------------------------------
for _dn, _dt in DT.items():
    for _xn, _xp in (("none", ()), ("the first", (0,)), ("the last", (2,)), ("all", (0, 1, 2))):
        for _e in ("bwd_dq", "bwd_dkv", "bwd"):
            case(f"{_e} {_dn} x 3, dS / Pd of {_xn}")(
                lambda L, e=_e, dt=_dt, xp=_xp: attn(L, e, dt, n=3, T=[(2, 64), (65, 128), (64, 64)], xp=xp))
case("fwd with dS / Pd set")(lambda L: attn(L, "fwd", S=128, xp=(0,)))

# ---------------------------------------------------------------------------------------------------------------------
# groups: 1, 2, 16 and BPM_MAX_GROUP problems of mixed sizes; none, one short of the limit, one past it; no array
# ---------------------------------------------------------------------------------------------------------------------
MIXED = [(65, 129), (1, 1), (64, 64), (129, 63), (512, 512), (2, 300)]
for _e in PLAIN + MASKED + MAPS:
    for _n in (1, 2, 16, MAX_GROUP):
        case(f"{_e}: {_n} mixed problems")(lambda L, e=_e, n=_n: attn(L, e, n=n, T=MIXED, per_head=(1,) if e.endswith("hmask") else ()))
    for _n in (0, 17, MAX_GROUP + 1):
        case(f"{_e}: {_n} problems")(lambda L, e=_e, n=_n: attn(L, e, n=n))
    case(f"{_e}: no problem array")(lambda L, e=_e: attn(L, e, probs=None))
    if kind_of(_e):
        case(f"{_e}: no mask array")(lambda L, e=_e: attn(L, e, masks=None))
for _n in (1, 2, 16, MAX_GROUP):
    case(f"bwd_dbias: {_n} mixed problems")(lambda L, n=_n: dbias(L, n=n, T=MIXED, per_head=(1,), out_heads=(1, 2)))
    case(f"bwd_dbias_ws_bytes: {_n} mixed problems")(lambda L, n=_n: dbias(L, n=n, T=MIXED, out_heads=(1, 2), query=True))
for _n in (0, 17, MAX_GROUP + 1):
    case(f"bwd_dbias: {_n} problems")(lambda L, n=_n: dbias(L, n=n))
    case(f"bwd_dbias_ws_bytes: {_n} problems")(lambda L, n=_n: dbias(L, n=n, query=True))
case("bwd_dbias: no output array")(lambda L: dbias(L, outs=None))
case("bwd_dbias: no mask array")(lambda L: dbias(L, masks=None))
case("bwd_dbias_ws_bytes: no output array")(lambda L: dbias(L, outs=None, query=True))

# ---------------------------------------------------------------------------------------------------------------------
# maps: both sides of one 64-query tile; one image for all heads against one per head
# ---------------------------------------------------------------------------------------------------------------------
for _dn, _dt in DT.items():
    for _T in (63, 64, 65, 128, 129):
        for _S in (65,):
            for _e in MAPS:
                case(f"{_e} {_dn} T={_T} S={_S}")(lambda L, e=_e, dt=_dt, T=_T, S=_S: attn(L, e, dt, T=T, S=S))
    case(f"maps_hmask {_dn} per head")(lambda L, dt=_dt: attn(L, "maps_hmask", dt, per_head=(0,)))
    case(f"maps_hmask {_dn} x 3, per head in the last")(lambda L, dt=_dt: attn(L, "maps_hmask", dt, n=3, T=MIXED, per_head=(2,)))
    case(f"maps_hmask {_dn} head stride of the forward image only")(
        lambda L, dt=_dt: attn(L, "maps_hmask", dt, edit=setm(0, head_stride=65 * 132)))

# ---------------------------------------------------------------------------------------------------------------------
# bias gradient: tiles on both sides of the split target (256 x 4 / 3 / 3 / 2 workgroups at head_dim 32 / 64 / 128 / 256),
# heads per image on both sides of DB_MIN_TERMS = 4, the workspace
# ---------------------------------------------------------------------------------------------------------------------
AT_TARGET = {32: (2048, 2048), 64: (1536, 2048), 128: (1536, 2048), 256: (1024, 2048)}
for _d, (_T, _S) in AT_TARGET.items():
    for _dn, _dt in DT.items():
        for _s in (_S, _S - 64, _S - 63):
            case(f"bwd_dbias {_dn} dhp={_d} T={_T} S={_s}")(lambda L, dt=_dt, d=_d, T=_T, S=_s: dbias(L, dt, dhp=d, T=T, S=S))
    case(f"bwd_dbias_ws_bytes dhp={_d} T={_T} S={_S - 64}")(lambda L, d=_d, T=_T, S=_S: dbias(L, dhp=d, T=T, S=S - 64, query=True))
    case(f"bwd_dbias_ws_bytes dhp={_d} T={_T} S={_S}")(lambda L, d=_d, T=_T, S=_S: dbias(L, dhp=d, T=T, S=S, query=True))
for _terms in (1, 3, 4, 5, 8, 9, 96):
    case(f"bwd_dbias one image, {_terms} heads")(lambda L, t=_terms: dbias(L, B=1, H=t))
    case(f"bwd_dbias_ws_bytes one image, {_terms} heads")(lambda L, t=_terms: dbias(L, B=1, H=t, query=True))
    case(f"bwd_dbias per head, {_terms} samples")(lambda L, t=_terms: dbias(L, B=t, H=2, per_head=(0,), out_heads=(0,)))
    case(f"bwd_dbias_ws_bytes per head, {_terms} samples")(lambda L, t=_terms: dbias(L, B=t, H=2, out_heads=(0,), query=True))
for _ws in ("none", "short", "misaligned"):
    case(f"bwd_dbias workspace {_ws}, needed")(lambda L, ws=_ws: dbias(L, B=2, H=8, ws=ws))
    case(f"bwd_dbias workspace {_ws}, not needed")(lambda L, ws=_ws: dbias(L, B=1, H=3, ws=ws))

# ---------------------------------------------------------------------------------------------------------------------
# refusals: one case per branch
# ---------------------------------------------------------------------------------------------------------------------
GEOMETRY = {
    "B=0": dict(B=0), "H=0": dict(H=0), "T=0": dict(T=0), "S=0": dict(S=0), "dh=0": dict(dh=0), "dh > dhp": dict(dh=65),
    "T=2^22": dict(T=1 << 22, mask_off=0), "T over 2^22": dict(T=(1 << 22) + 1, mask_off=0), "S over 2^22": dict(S=(1 << 22) + 1, mask_off=0),
    "q_pos0 < 0": dict(q_pos0=-1), "q_stride < 0": dict(q_stride=-1), "q_pos0=2^24": dict(q_pos0=1 << 24),
    "q_pos0 over 2^24": dict(q_pos0=(1 << 24) + 1), "q_stride=2^24": dict(q_stride=1 << 24, T=17),
    "q_stride over 2^24": dict(q_stride=(1 << 24) + 1, T=2), "last position 2^28": dict(q_stride=1 << 18, T=1025),
    "last position over 2^28": dict(q_stride=1 << 18, T=1025, q_pos0=1), "mask_off over 2^29": dict(mask_off=(1 << 29) + 1),
}
for _e in ("fwd", "bwd_dkv_kmask", "maps_amask"):
    for _gn, _g in GEOMETRY.items():
        case(f"{_e}: {_gn}")(lambda L, e=_e, g=_g: attn(L, e, edit=setp(0, **g)))
    case(f"{_e}: mixed dhp")(lambda L, e=_e: attn(L, e, n=2, edit=setp(1, dhp=128)))
    case(f"{_e}: dhp=256, 2^21 rows")(lambda L, e=_e: attn(L, e, dhp=256, edit=setp(0, T=1 << 21, mask_off=0)))
    case(f"{_e}: dhp=256, 2^21 + 1 rows")(lambda L, e=_e: attn(L, e, dhp=256, edit=setp(0, S=(1 << 21) + 1, mask_off=0)))
for _gn, _g in GEOMETRY.items():
    case(f"bwd_dbias: {_gn}")(lambda L, g=_g: dbias(L, edit=setp(0, **g)))
case("bwd_dbias: mixed dhp")(lambda L: dbias(L, n=2, edit=setp(1, dhp=128)))
case("bwd_dbias: dhp=256, 2^21 + 1 rows")(lambda L: dbias(L, dhp=256, edit=setp(0, S=(1 << 21) + 1, mask_off=0)))

# the pointers each kernel needs (and the ones it does not)
for _f in ("Q", "K", "V", "O", "lse", "dO", "delta", "dQ", "dK", "dV"):
    for _e in PLAIN + MASKED:
        case(f"{_e}: no {_f}")(lambda L, e=_e, f=_f: attn(L, e, edit=setp(0, **{f: None})))
    case(f"bwd: no {_f} in the second problem")(lambda L, f=_f: attn(L, "bwd", n=2, edit=setp(1, **{f: None})))
    case(f"bwd_dbias: no {_f}")(lambda L, f=_f: dbias(L, edit=setp(0, **{f: None})))
for _f in ("Q", "K", "lse", "W"):
    for _e in MAPS:
        case(f"{_e}: no {_f}")(lambda L, e=_e, f=_f: attn(L, e, edit=setp(0, **{f: None})))

# the dS / Pd rules of the dQ pass
XP_FAULTS = {
    "dS without Pd": dict(Pd=None), "Pd without dS": dict(dS=None), "S not a multiple of 4": dict(S=126),
    "xs_b not a multiple of 4": dict(xs_b=3 * 65 * 128 + 2), "xs_h not a multiple of 4": dict(xs_h=65 * 128 + 1),
    "xs_q not a multiple of 4": dict(xs_q=130), "xs_b < 0": dict(xs_b=-4), "xs_h < 0": dict(xs_h=-4), "xs_q < S": dict(xs_q=124),
    "dS 8 bytes off": dict(dS=BASE + (1 << 42) + 8), "Pd 4 bytes off": dict(Pd=BASE + (1 << 42) + 4),
}
for _xn, _x in XP_FAULTS.items():
    for _e in ("bwd_dq", "fwd"):
        case(f"{_e}: {_xn}")(lambda L, e=_e, x=_x: attn(L, e, S=128, xp=(0,), edit=setp(0, **x)))
for _e in MASKED:
    case(f"{_e}: dS / Pd set")(lambda L, e=_e: attn(L, e, S=128, xp=(0,)))
case("bwd_dbias: dS / Pd set")(lambda L: dbias(L, S=128, xp=(0,)))
case("bwd_dbias: Pd alone set")(lambda L: dbias(L, S=128, edit=setp(0, Pd=BASE + (1 << 42))))

# per-key masks
for _e in MASKED[:3]:
    case(f"{_e}: null mask")(lambda L, e=_e: attn(L, e, edit=setm(0, mask=None)))
    case(f"{_e}: null mask in the second problem")(lambda L, e=_e: attn(L, e, n=2, edit=setm(1, mask=None)))
    case(f"{_e}: ldm < S")(lambda L, e=_e: attn(L, e, edit=setm(0, ldm=128)))
    case(f"{_e}: ldm = S + 1")(lambda L, e=_e: attn(L, e, edit=setm(0, ldm=130)))

# additive masks, one image or one per head (T 65, S 129: ldm 132, ldt 68)
AM_FAULTS = {
    "null mask": dict(mask=None), "ldm < S": dict(ldm=128), "ldm not a multiple of 4": dict(ldm=134), "mask 8 bytes off": dict(mask=BASE + (1 << 42) + 8),
    "null maskT": dict(maskT=None), "ldt < T": dict(ldt=64), "ldt not a multiple of 4": dict(ldt=70), "maskT 4 bytes off": dict(maskT=BASE + (1 << 42) + 4),
}
HS_FAULTS = {
    "head stride short": dict(head_stride=65 * 132 - 4), "head stride not a multiple of 4": dict(head_stride=65 * 132 + 2),
    "head stride over 31 bits": dict(head_stride=1 << 31), "head stride 2^31 - 4": dict(head_stride=(1 << 31) - 4),
    "head strideT short": dict(head_strideT=129 * 68 - 4), "head strideT not a multiple of 4": dict(head_strideT=129 * 68 + 2),
    "head strideT over 31 bits": dict(head_strideT=1 << 31), "head strideT alone": dict(head_strideT=129 * 68),
}
for _fn, _f in AM_FAULTS.items():
    for _e in ("fwd_amask", "bwd_dkv_amask", "bwd_dq_hmask", "bwd_dkv_hmask", "maps_amask"):
        case(f"{_e}: {_fn}")(lambda L, e=_e, f=_f: attn(L, e, edit=setm(0, **f)))
    case(f"bwd_dbias: {_fn}")(lambda L, f=_f: dbias(L, edit=setm(0, **f)))
for _fn, _f in HS_FAULTS.items():
    for _e in MASKED[6:] + MAPS[2:]:
        case(f"{_e}: {_fn}")(lambda L, e=_e, f=_f: attn(L, e, per_head=(0,), edit=setm(0, **f)))
    case(f"bwd_dbias: {_fn}")(lambda L, f=_f: dbias(L, per_head=(0,), edit=setm(0, **f)))

# maps
for _e in MAPS:
    case(f"{_e}: ldw < S")(lambda L, e=_e: attn(L, e, edit=setp(0, ldw=128)))
    case(f"{_e}: Q 8 bytes off")(lambda L, e=_e: attn(L, e, edit=setp(0, Q=BASE + (1 << 42) + 8)))
    case(f"{_e}: K 8 bytes off")(lambda L, e=_e: attn(L, e, edit=setp(0, K=BASE + (1 << 42) + 8)))
    case(f"{_e}: lse 2 bytes off")(lambda L, e=_e: attn(L, e, edit=setp(0, lse=BASE + (1 << 42) + 2)))
    case(f"{_e}: W 2 bytes off")(lambda L, e=_e: attn(L, e, edit=setp(0, W=BASE + (1 << 42) + 2)))
    case(f"{_e}: W 4 bytes off")(lambda L, e=_e: attn(L, e, edit=setp(0, W=BASE + (1 << 42) + 4)))
    case(f"{_e}: 2^30 blocks")(lambda L, e=_e: attn(L, e, B=1, H=1, edit=both(setp(0, T=1 << 21, S=1 << 21, ldw=1 << 21, mask_off=0),
                                                                                  setm(0, ldm=1 << 21, ldt=1 << 21) if kind_of(e) else setp(0))))
    case(f"{_e}: over 2^30 blocks")(lambda L, e=_e: attn(L, e, B=2, H=1, edit=both(setp(0, T=1 << 21, S=1 << 21, ldw=1 << 21, mask_off=0),
                                                                                       setm(0, ldm=1 << 21, ldt=1 << 21) if kind_of(e) else setp(0))))

# bias gradient
DB_FAULTS = {
    "null dB": dict(dB=None), "lddb < S": dict(lddb=128), "lddb not a multiple of 4": dict(lddb=131), "lddb = S + 1": dict(lddb=130),
    "dB 8 bytes off": dict(dB=BASE + (1 << 42) + 8), "output head stride short": dict(head_stride=65 * 132 - 4),
    "output head stride not a multiple of 4": dict(head_stride=65 * 132 + 2), "output head stride 2^31": dict(head_stride=1 << 31),
}
for _fn, _f in DB_FAULTS.items():
    case(f"bwd_dbias: {_fn}")(lambda L, f=_f: dbias(L, edit=seto(0, **f)))
    case(f"bwd_dbias_ws_bytes: {_fn}")(lambda L, f=_f: dbias(L, edit=seto(0, **f), query=True))
for _f in ("Q", "K", "V", "dO"):
    case(f"bwd_dbias: {_f} 8 bytes off")(lambda L, f=_f: dbias(L, edit=setp(0, **{f: BASE + (1 << 42) + 8})))
case("bwd_dbias: over 2^30 blocks")(lambda L: dbias(L, B=1, H=1, out_heads=(0,), edit=both(
    setp(0, T=1 << 21, S=(1 << 21) + 64, mask_off=0), setm(0, ldm=(1 << 21) + 64, ldt=1 << 21), seto(0, lddb=(1 << 21) + 64, head_stride=1 << 43))))

# ---------------------------------------------------------------------------------------------------------------------
# two faults with different codes: the order of the tests decides
# ---------------------------------------------------------------------------------------------------------------------
OFF = BASE + (1 << 42) + 8
for _e in ("fwd", "bwd", "bwd_dq_kmask", "fwd_amask"):
    case(f"{_e}: no Q in the first problem, dS misaligned in the second")(
        lambda L, e=_e: attn(L, e, n=2, S=128, xp=(1,), edit=both(setp(0, Q=None), setp(1, dS=OFF))))
    case(f"{_e}: dS misaligned in the first problem, T=0 in the second")(
        lambda L, e=_e: attn(L, e, n=2, S=128, xp=(0,), edit=both(setp(0, dS=OFF), setp(1, T=0))))
    case(f"{_e}: T=0 in the first problem, dS misaligned in the second")(
        lambda L, e=_e: attn(L, e, n=2, S=128, xp=(1,), edit=both(setp(0, T=0), setp(1, dS=OFF))))
    case(f"{_e}: dS misaligned and xs_q < S")(lambda L, e=_e: attn(L, e, S=128, xp=(0,), edit=setp(0, dS=OFF, xs_q=124)))
case("bwd_dq_kmask: dtype 7, dS misaligned")(lambda L: attn(L, "bwd_dq_kmask", 7, S=128, xp=(0,), edit=setp(0, dS=OFF)))
case("fwd_hmask: dS misaligned, null mask")(lambda L: attn(L, "fwd_hmask", S=128, xp=(0,), edit=both(setp(0, dS=OFF), setm(0, mask=None))))
for _e in MAPS:
    case(f"{_e}: Q misaligned and q_pos0 < 0")(lambda L, e=_e: attn(L, e, edit=setp(0, Q=OFF, q_pos0=-1)))
    case(f"{_e}: Q misaligned and ldw < S")(lambda L, e=_e: attn(L, e, edit=setp(0, Q=OFF, ldw=128)))
    case(f"{_e}: q_pos0 < 0 in the first problem, Q misaligned in the second")(
        lambda L, e=_e: attn(L, e, n=2, edit=both(setp(0, q_pos0=-1), setp(1, Q=OFF))))
    case(f"{_e}: Q misaligned in the first problem, no W in the second")(
        lambda L, e=_e: attn(L, e, n=2, edit=both(setp(0, Q=OFF), setp(1, W=None))))
    case(f"{_e}: Q misaligned, dhp=48")(lambda L, e=_e: attn(L, e, dhp=48, edit=setp(0, Q=OFF)))
case("maps_amask: Q misaligned, null maskT")(lambda L: attn(L, "maps_amask", edit=both(setp(0, Q=OFF), setm(0, maskT=None))))
case("bwd_dbias: Q misaligned, null mask")(lambda L: dbias(L, edit=both(setp(0, Q=OFF), setm(0, mask=None))))
case("bwd_dbias: Q misaligned, no lse")(lambda L: dbias(L, edit=setp(0, Q=OFF, lse=None)))
case("bwd_dbias: Q misaligned, q_pos0 < 0")(lambda L: dbias(L, edit=setp(0, Q=OFF, q_pos0=-1)))
case("bwd_dbias: Q misaligned, no workspace")(lambda L: dbias(L, B=2, H=8, ws="none", edit=setp(0, Q=OFF)))
case("bwd_dbias: Q misaligned, lddb < S")(lambda L: dbias(L, edit=both(setp(0, Q=OFF), seto(0, lddb=128))))
case("bwd_dbias: no mask in the first problem, Q misaligned in the second")(
    lambda L: dbias(L, n=2, edit=both(setm(0, mask=None), setp(1, Q=OFF))))
