"""The case table of tests/test_rowops_dispatch_cpu.py: calls of the row-kernel and Adam entry points at made-up aligned
addresses, and the runner that asks a -DBPM_LAB build which launches each call makes (bpm_debug_rows_dry: nothing is
launched, nothing is dereferenced).  tools/rowops_dispatch.py runs the same table against any lab build and writes the
record the test compares with (profiles/rowops_dispatch.json, recorded from the tree before csrc/rowops.hip was split).

A case is name -> function(L) -> return code of the entry.  Its record is {"rc": code, "launches": [[kernel, grid, block,
aux], ...]}: kernel normalised to `name<args>`, aux the launch's last pointer argument (the LayerNorm workspace, Adam's
step counters, ...) or 0."""
import ctypes as C
import re

from bpmult_amd import _lib
from bpmult_amd._lib import BPM_BF16 as BF, BPM_F32 as F32, MAX_GROUP

BASE = 0x7F0000000000
DT = {"bf16": BF, "f32": F32}
CASES = {}


class Addr:
    """Made-up device addresses, 256 MB apart."""

    def __init__(self):
        self.next = BASE

    def __call__(self, off=0):
        a = self.next
        self.next += 1 << 28
        return a + off


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


MANGLED_ARG = {"f": "float", "DF16b": "bf16_t", "Lb0E": "false", "Lb1E": "true"}


def normalise(kernel: str) -> str:
    """`name<args>` from either spelling a build records: the source text of a launch's first argument
    (`(ln_fwd_vec_kernel<bf16_t, 3>)`), or the mangled name of a type that carries the kernel as a template argument
    (`...9KernelTagIXadL_ZNS_17ln_fwd_vec_kernelIDF16bLi3EEEvNS_3GrpINS_3LnPEEEifEEEE`)."""
    m = re.search(r"KernelTagIXadL_Z(?:NS_)?\d+(\w+?_kernel)(?:I((?:DF16b|f|Li\d+E|Lb[01]E)+)E)?", kernel)
    if not m:
        return re.sub(r"\s+", "", kernel).strip("()")
    args = [MANGLED_ARG.get(a) or a[2:-1] for a in re.findall(r"DF16b|f|Li\d+E|Lb[01]E", m.group(2) or "")]
    return m.group(1) + ("<" + ",".join(args) + ">" if args else "")


def run(L, fn):
    """L: a -DBPM_LAB build with its hooks bound (_lib.lab_library / _lib.bind_lab)"""
    L.bpm_debug_rows_dry(1)
    try:
        rc = fn(L)
        launches = []
        name, grid, block, aux = C.create_string_buffer(512), C.c_uint(), C.c_uint(), C.c_void_p()
        n = L.bpm_debug_rows_last(-1, None, 0, None, None, None)
        for i in range(n):
            L.bpm_debug_rows_last(i, name, 512, C.byref(grid), C.byref(block), C.byref(aux))
            launches.append([normalise(name.value.decode()), grid.value, block.value, aux.value or 0])
    finally:
        L.bpm_debug_rows_dry(0)
    return {"rc": rc, "launches": launches}


def run_all(L):
    return {name: run(L, fn) for name, fn in CASES.items()}


# ---------------------------------------------------------------------------------------------------------------------
# LayerNorm
# ---------------------------------------------------------------------------------------------------------------------
def ln_problems(d, n=1, R=64, ldo=None, out_f32=0, x_off=0, bwd=False, cast_ldc=0, csum=False, dgamma=True, share=False,
                dbeta_off=0, drop_p=0.0):
    A = Addr()
    q = (_lib.LnProblem * n)()
    shared = A()
    for i, p in enumerate(q):
        p.x, p.gamma, p.beta, p.mean, p.rstd, p.R = A(x_off), A(), A(), A(), A(), R
        if bwd:
            p.dy, p.ldy, p.add, p.dx = A(), d, A(), A()
            if dgamma:
                p.dgamma, p.dbeta = (shared if share else A()), A(dbeta_off)
            if cast_ldc:
                p.cast, p.ldc, p.drop_p, p.drop_site = A(), cast_ldc, drop_p, 7 + i
                if csum:
                    p.cast_colsum = A()
        else:
            p.out, p.ldo, p.out_f32 = A(), d if ldo is None else ldo, out_f32
    return q


for _dn, _dt in DT.items():
    for _d in (24, 50, 300, 768, 770, 1024, 1028, 1536, 2048, 2049):
        case(f"ln_fwd {_dn} d={_d}")(lambda L, dt=_dt, d=_d: L.bpm_ln_fwd(dt, ln_problems(d), 1, d, 1e-5, None))
    case(f"ln_fwd {_dn} d=768, x 4 bytes off")(lambda L, dt=_dt: L.bpm_ln_fwd(dt, ln_problems(768, x_off=4), 1, 768, 1e-5, None))
    case(f"ln_fwd {_dn} d=40 ldo=64")(lambda L, dt=_dt: L.bpm_ln_fwd(dt, ln_problems(40, ldo=64), 1, 40, 1e-5, None))
    case(f"ln_fwd {_dn} d=256 ldo=288")(lambda L, dt=_dt: L.bpm_ln_fwd(dt, ln_problems(256, ldo=288), 1, 256, 1e-5, None))
    case(f"ln_fwd {_dn} d=256 ldo=288 out_f32")(lambda L, dt=_dt: L.bpm_ln_fwd(dt, ln_problems(256, ldo=288, out_f32=1), 1, 256, 1e-5, None))
    case(f"ln_fwd {_dn} d=768 out_f32")(lambda L, dt=_dt: L.bpm_ln_fwd(dt, ln_problems(768, out_f32=1), 1, 768, 1e-5, None))
    for _R in (1, 16384, 16388):
        case(f"ln_fwd {_dn} d=768 rows={_R} x 3")(lambda L, dt=_dt, R=_R: L.bpm_ln_fwd(dt, ln_problems(768, n=3, R=R), 3, 768, 1e-5, None))
        case(f"ln_fwd {_dn} d=50 rows={_R}")(lambda L, dt=_dt, R=_R: L.bpm_ln_fwd(dt, ln_problems(50, R=R), 1, 50, 1e-5, None))


def ln_bwd(L, dt, d, n=1, ws="fits", entry="ws", **kw):
    q = ln_problems(d, n=n, bwd=True, **kw)
    if entry == "plain":
        return L.bpm_ln_bwd(dt, q, n, d, 5, None)
    vec_blocks = sum(min(64, max(1, (p.R + 7) // 8)) for p in q)
    need = (vec_blocks * 3 * d + 64) * 4
    wsp = None if ws == "none" else BASE - (1 << 30)
    return L.bpm_ln_bwd_ws(dt, q, n, d, 5, wsp, need - 4 if ws == "short" else need, None)


for _dn, _dt in DT.items():
    for _R in (8, 512, 520):
        case(f"ln_bwd_ws {_dn} d=768 rows={_R} x 2")(lambda L, dt=_dt, R=_R: ln_bwd(L, dt, 768, n=2, R=R))
    for _R in (4, 1024, 1028):
        case(f"ln_bwd_ws {_dn} d=50 rows={_R} x 2")(lambda L, dt=_dt, R=_R: ln_bwd(L, dt, 50, n=2, R=R))
    for _d in (24, 256, 260, 300, 768, 772, 1024, 1028, 770, 2048, 2049):
        case(f"ln_bwd_ws {_dn} d={_d}")(lambda L, dt=_dt, d=_d: ln_bwd(L, dt, d))
    case(f"ln_bwd_ws {_dn} d=1000 ldc=1024")(lambda L, dt=_dt: ln_bwd(L, dt, 1000, cast_ldc=1024, csum=True, drop_p=0.1))
    case(f"ln_bwd_ws {_dn} d=768 cast, no column sums")(lambda L, dt=_dt: ln_bwd(L, dt, 768, cast_ldc=768))
    case(f"ln_bwd_ws {_dn} d=768 no sums at all")(lambda L, dt=_dt: ln_bwd(L, dt, 768, dgamma=False))
    case(f"ln_bwd_ws {_dn} d=768 cast sums only")(lambda L, dt=_dt: ln_bwd(L, dt, 768, dgamma=False, cast_ldc=768, csum=True))
    case(f"ln_bwd_ws {_dn} d=768 shared dgamma")(lambda L, dt=_dt: ln_bwd(L, dt, 768, n=2, share=True))
    case(f"ln_bwd_ws {_dn} d=768 dbeta 4 bytes off")(lambda L, dt=_dt: ln_bwd(L, dt, 768, dbeta_off=4))
    case(f"ln_bwd_ws {_dn} d=768 workspace one float short")(lambda L, dt=_dt: ln_bwd(L, dt, 768, n=2, ws="short"))
    case(f"ln_bwd_ws {_dn} d=768 no sums, workspace short")(lambda L, dt=_dt: ln_bwd(L, dt, 768, dgamma=False, ws="short"))
    case(f"ln_bwd_ws {_dn} d=768 null workspace")(lambda L, dt=_dt: ln_bwd(L, dt, 768, ws="none"))
    case(f"ln_bwd_ws {_dn} d=768 x 4 bytes off")(lambda L, dt=_dt: ln_bwd(L, dt, 768, x_off=4))
    case(f"ln_bwd {_dn} d=768")(lambda L, dt=_dt: ln_bwd(L, dt, 768, entry="plain"))
    case(f"ln_bwd {_dn} d=50")(lambda L, dt=_dt: ln_bwd(L, dt, 50, entry="plain"))
case("ln_bwd_ws dtype 2")(lambda L: ln_bwd(L, 2, 768))


# ---------------------------------------------------------------------------------------------------------------------
# key / value source
# ---------------------------------------------------------------------------------------------------------------------
def kv_problems(d, n=1, T=8, B=8, ld=None, same=True, all_but_one=False, bwd=False):
    A = Addr()
    q = (_lib.KvSourceProblem * n)()
    for i, p in enumerate(q):
        p.xk = A()
        p.xv = p.xk if same or (all_but_one and i > 0) else A()
        p.T, p.B, p.pos0, p.pos_stride = T, B, 0, 1
        p.drop_p_k, p.drop_site_k, p.drop_p_v, p.drop_site_v = 0.25, 2 * i, 0.25, 2 * i + 1
        p.mean_k, p.rstd_k, p.mean_v, p.rstd_v = A(), A(), A(), A()
        if bwd:
            p.gk, p.gv, p.dxk, p.dxv = A(), A(), A(), A()
        else:
            p.khat, p.vhat, p.ld = A(), A(), d if ld is None else ld
    return q, A(), T + 2


def kv_fwd(L, dt, d, n=1, **kw):
    q, table, rows = kv_problems(d, n=n, **kw)
    return L.bpm_kv_source_fwd(dt, q, n, table, rows, d, 2.0, 1e-5, 5, None)


def kv_bwd(L, d, n=1, **kw):
    q, table, rows = kv_problems(d, n=n, bwd=True, **kw)
    return L.bpm_kv_source_bwd(q, n, table, rows, d, 2.0, 5, None)


for _d in (256, 260, 768, 1024, 1028):
    for _dn, _dt in DT.items():
        case(f"kv_source_fwd {_dn} d={_d}")(lambda L, dt=_dt, d=_d: kv_fwd(L, dt, d))
    case(f"kv_source_bwd d={_d}")(lambda L, d=_d: kv_bwd(L, d))
    case(f"kv_source_bwd d={_d}, xk != xv")(lambda L, d=_d: kv_bwd(L, d, same=False))
for _dn, _dt in DT.items():
    case(f"kv_source_fwd {_dn} d=256 ld=288")(lambda L, dt=_dt: kv_fwd(L, dt, 256, ld=288))
    case(f"kv_source_fwd {_dn} d=768, xk != xv")(lambda L, dt=_dt: kv_fwd(L, dt, 768, same=False))
case("kv_source_fwd dtype 2")(lambda L: kv_fwd(L, 2, 768))
case("kv_source_bwd d=768 x 3, xk != xv in one")(lambda L: kv_bwd(L, 768, n=3, same=False, all_but_one=True))
case("kv_source_bwd d=768 x 3, xk == xv in all")(lambda L: kv_bwd(L, 768, n=3))
for _T, _B in ((1, 1), (4096, 4), (4097, 4), (8192, 4), (8194, 4)):
    case(f"kv_source_fwd bf16 d=64 T={_T} B={_B} x 2")(lambda L, T=_T, B=_B: kv_fwd(L, BF, 64, n=2, T=T, B=B))
    case(f"kv_source_bwd d=64 T={_T} B={_B} x 2")(lambda L, T=_T, B=_B: kv_bwd(L, 64, n=2, T=T, B=B))
    case(f"kv_source_bwd d=64 T={_T} B={_B} x 2, xk != xv")(lambda L, T=_T, B=_B: kv_bwd(L, 64, n=2, T=T, B=B, same=False))


# ---------------------------------------------------------------------------------------------------------------------
# rows_cast
# ---------------------------------------------------------------------------------------------------------------------
def cast(L, dt, R, Cc, n=1, lda=None, ct=True, f32=False, colsum=False, b=False, drop_p=0.0, a_is_ct=0, a_off=0):
    A = Addr()
    q = (_lib.CastProblem * n)()
    for i, p in enumerate(q):
        p.a, p.lda, p.a_is_ct, p.R, p.C = A(a_off), Cc if lda is None else lda, a_is_ct, R, Cc
        if b:
            p.b, p.ldb = A(), Cc
        if ct:
            p.dst_ct, p.ldd = A(), (Cc + 31) // 32 * 32
        if f32:
            p.dst_f32, p.ldf = A(), Cc
        if colsum:
            p.colsum = A()
        p.drop_p, p.drop_site = drop_p, i
    return L.bpm_rows_cast(dt, q, n, 5, None)


for _dn, _dt in DT.items():
    case(f"rows_cast {_dn} plain cast 100 x 300")(lambda L, dt=_dt: cast(L, dt, 100, 300))
    case(f"rows_cast {_dn} cast + f32 + column sums + dropout")(lambda L, dt=_dt: cast(L, dt, 100, 300, f32=True, colsum=True, drop_p=0.1))
    for _R in (32, 33):
        case(f"rows_cast {_dn} cast rows={_R} C=300 x 2")(lambda L, dt=_dt, R=_R: cast(L, dt, R, 300, n=2))
    for _R in (128, 129):
        case(f"rows_cast {_dn} column sums rows={_R} C=768 x 2")(lambda L, dt=_dt, R=_R: cast(L, dt, R, 768, n=2, ct=False, colsum=True))
    case(f"rows_cast {_dn} column sums C=1024")(lambda L, dt=_dt: cast(L, dt, 200, 1024, ct=False, colsum=True))
    case(f"rows_cast {_dn} column sums C=1028")(lambda L, dt=_dt: cast(L, dt, 200, 1028, ct=False, colsum=True))
    case(f"rows_cast {_dn} column sums C=30 lda=32")(lambda L, dt=_dt: cast(L, dt, 200, 30, lda=32, ct=False, colsum=True))
    case(f"rows_cast {_dn} column sums C=30 lda=30")(lambda L, dt=_dt: cast(L, dt, 200, 30, ct=False, colsum=True))
    case(f"rows_cast {_dn} column sums lda=770")(lambda L, dt=_dt: cast(L, dt, 200, 768, lda=770, ct=False, colsum=True))
    case(f"rows_cast {_dn} column sums with dropout")(lambda L, dt=_dt: cast(L, dt, 200, 768, ct=False, colsum=True, drop_p=0.1))
    case(f"rows_cast {_dn} column sums with b")(lambda L, dt=_dt: cast(L, dt, 200, 768, ct=False, colsum=True, b=True))
    case(f"rows_cast {_dn} column sums of a CT matrix")(lambda L, dt=_dt: cast(L, dt, 200, 768, ct=False, colsum=True, a_is_ct=1))
    case(f"rows_cast {_dn} column sums of a CT matrix 8 bytes off")(lambda L, dt=_dt: cast(L, dt, 200, 768, ct=False, colsum=True, a_is_ct=1, a_off=8))
    case(f"rows_cast {_dn} column sums, a 8 bytes off")(lambda L, dt=_dt: cast(L, dt, 200, 768, ct=False, colsum=True, a_off=8))
    case(f"rows_cast {_dn} column sums beside a cast")(lambda L, dt=_dt: cast(L, dt, 200, 768, colsum=True))
case("rows_cast nothing to write")(lambda L: cast(L, BF, 100, 300, ct=False))


# ---------------------------------------------------------------------------------------------------------------------
# element-wise entries: 1024 elements (256 four-element chunks) per block, at most 2048 blocks per problem
# ---------------------------------------------------------------------------------------------------------------------
def pack_rows(L, dt, B, T, Cc, n=1, bwd=False):
    A = Addr()
    q = (_lib.PackProblem * n)()
    for i, p in enumerate(q):
        p.B, p.T, p.C, p.ld, p.ldg, p.drop_p, p.drop_site = B, T, Cc, Cc, Cc, 0.1, i
        if bwd:
            p.g, p.dsrc = A(), A()
        else:
            p.src, p.dst = A(), A()
    return L.bpm_pack_rows_bwd(q, n, 5, None) if bwd else L.bpm_pack_rows_fwd(dt, q, n, 5, None)


def embed(L, T, B, d, n=1, bwd=False):
    A = Addr()
    q = (_lib.EmbedProblem * n)()
    for i, p in enumerate(q):
        p.x, p.out, p.T, p.B, p.drop_p, p.drop_site = A(), A(), T, B, 0.1, i
    return L.bpm_embed_pos_bwd(q, n, d, 2.0, 5, None) if bwd else L.bpm_embed_pos_fwd(q, n, A(), T + 2, d, 2.0, 5, None)


def gmu(L, dt, R, d, n=1, bwd=False):
    A = Addr()
    q = (_lib.GmuProblem * n)()
    for p in q:
        p.a1, p.a2, p.ag, p.x1, p.x2, p.out, p.R = A(), A(), A(), A(), A(), A(), R
        p.dout, p.da1, p.da2, p.dag, p.ldg, p.dx1, p.dx2 = A(), A(), A(), A(), d, A(), A()
    return L.bpm_gmu2_bwd(dt, q, n, d, None) if bwd else L.bpm_gmu2_fwd(q, n, d, None)


def gelu(L, dt, R, Cc, n=1, bwd=False):
    A = Addr()
    q = (_lib.GeluProblem * n)()
    for p in q:
        p.u, p.ldu, p.g, p.ldg, p.dg, p.lddg, p.du, p.lddu, p.R, p.C = A(), Cc, A(), Cc, A(), Cc, A(), Cc, R, Cc
    return (L.bpm_gelu_bwd if bwd else L.bpm_gelu_fwd)(dt, q, n, None)


def split(L, R, Cc, n=1):
    A = Addr()
    q = (_lib.SplitProblem * n)()
    for p in q:
        p.src, p.dst, p.R, p.C, p.ld, p.ldp = A(), A(), R, Cc, Cc, Cc
    return L.bpm_split_rows(q, n, None)


def add_n(L, count, n=1, n_in=3):
    A = Addr()
    q = (_lib.AddnProblem * n)()
    for p in q:
        p.out, p.n_in, p.count = A(), n_in, count
        for j in range(n_in):
            p.src[j] = A()
    return L.bpm_add_n(q, n, None)


def expand(L, dt, H, n=1, dbias=True):
    A = Addr()
    q = (_lib.ExpandProblem * n)()
    for p in q:
        p.q, p.dO, p.qexp, p.dOexp, p.Pd = A(), A(), A(), A(), A()
        if dbias:
            p.dbias = A()
        p.B, p.H, p.T, p.S, p.dh, p.dhp, p.ld = 2, H, 8, 50, 64, 64, H * 64
    return L.bpm_expand_heads(dt, q, n, None)


# (rows, columns) with 4 | columns: 1 chunk / the cap of 2048 blocks / one block's worth past it / between
SIZES = {"one chunk": (1, 4), "two blocks": (257, 4), "2048 blocks": (2048, 1024), "2048 blocks + one row": (2049, 1024)}
for _sn, (_R, _C) in SIZES.items():
    for _dn, _dt in DT.items():
        case(f"pack_rows_fwd {_dn} {_sn} x 2")(lambda L, dt=_dt, R=_R, Cc=_C: pack_rows(L, dt, 1, R, Cc, n=2))
        case(f"gmu2_bwd {_dn} {_sn} x 2")(lambda L, dt=_dt, R=_R, Cc=_C: gmu(L, dt, R, Cc, n=2, bwd=True))
        case(f"gelu_fwd {_dn} {_sn} x 2")(lambda L, dt=_dt, R=_R, Cc=_C: gelu(L, dt, R, 4 * Cc, n=2))
        case(f"gelu_bwd {_dn} {_sn} x 2")(lambda L, dt=_dt, R=_R, Cc=_C: gelu(L, dt, R, 4 * Cc, n=2, bwd=True))
    case(f"pack_rows_bwd {_sn} x 2")(lambda L, R=_R, Cc=_C: pack_rows(L, BF, 1, R, Cc, n=2, bwd=True))
    case(f"embed_pos_fwd {_sn} x 2")(lambda L, R=_R, Cc=_C: embed(L, R, 1, Cc, n=2))
    case(f"embed_pos_bwd {_sn} x 2")(lambda L, R=_R, Cc=_C: embed(L, R, 1, Cc, n=2, bwd=True))
    case(f"gmu2_fwd {_sn} x 2")(lambda L, R=_R, Cc=_C: gmu(L, BF, R, Cc, n=2))
    case(f"split_rows {_sn} x 2")(lambda L, R=_R, Cc=_C: split(L, R, 4 * Cc, n=2))
    case(f"add_n {_sn} x 2")(lambda L, R=_R, Cc=_C: add_n(L, 4 * R * Cc, n=2))
case("add_n one element")(lambda L: add_n(L, 1))
case("pack_rows_fwd bf16 one element")(lambda L: pack_rows(L, BF, 1, 1, 1))
case("gelu_fwd dtype 2")(lambda L: gelu(L, 2, 4, 4))
case("gelu_fwd ld not a multiple of 4")(lambda L: gelu(L, BF, 4, 6))
for _dn, _dt in DT.items():
    case(f"expand_heads {_dn} 12 heads x 3")(lambda L, dt=_dt: expand(L, dt, 12, n=3))
    case(f"expand_heads {_dn} 1 head, no bias sums")(lambda L, dt=_dt: expand(L, dt, 1, dbias=False))
case("expand_heads dtype 2")(lambda L: expand(L, 2, 12))


# ---------------------------------------------------------------------------------------------------------------------
# table-driven entries: the table is device memory (never read by the host), total_blocks is the grid
# ---------------------------------------------------------------------------------------------------------------------
TAB = BASE + 0x1000
for _tb in (1, 777):
    for _dn, _dt in DT.items():
        case(f"pack_weights {_dn} {_tb} blocks")(lambda L, dt=_dt, tb=_tb: L.bpm_pack_weights(dt, TAB, 3, tb, None))
    case(f"fold_bias {_tb} blocks")(lambda L, tb=_tb: L.bpm_fold_bias(TAB, 3, tb, None))
    case(f"unfold_grads accumulate {_tb} blocks")(lambda L, tb=_tb: L.bpm_unfold_grads(TAB, 3, tb, 0, None))
    case(f"unfold_grads store {_tb} blocks")(lambda L, tb=_tb: L.bpm_unfold_grads(TAB, 3, tb, 1, None))
    case(f"zero_segments {_tb} blocks")(lambda L, tb=_tb: L.bpm_zero_segments(TAB, 3, tb, None))
    case(f"grad_sumsq {_tb} blocks")(lambda L, tb=_tb: L.bpm_grad_sumsq(TAB, 3, tb, 1.0, 0.8, None, BASE + 0x2000, (tb + 3) // 4 * 16, BASE + 0x3000, None))
case("pack_weights no blocks")(lambda L: L.bpm_pack_weights(BF, TAB, 3, 0, None))
case("fold_bias no table")(lambda L: L.bpm_fold_bias(None, 3, 5, None))
case("unfold_grads no descriptors")(lambda L: L.bpm_unfold_grads(TAB, 0, 5, 0, None))
case("zero_segments no blocks")(lambda L: L.bpm_zero_segments(TAB, 3, 0, None))
case("grad_sumsq workspace short")(lambda L: L.bpm_grad_sumsq(TAB, 3, 5, 1.0, 0.8, None, BASE + 0x2000, 16, BASE + 0x3000, None))

BUF = tuple(BASE + (k << 28) for k in range(1, 5))            # param, grad, exp_avg, exp_avg_sq
HYPER = (1e-3, 0.9, 0.999, 1e-8, 0.01)
SCALE, NORM, STEPS, SKIPPED = (BASE + 0x5000 + 0x100 * k for k in range(4))


def adam_groups(L, dt, tb, ngroups=2, **dev):
    g = (_lib.AdamGroup * ngroups)()
    for i, h in enumerate(g):
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled, h.step = 1e-3, 0.9, 0.999, 1e-8, 0.01, i & 1, 3
    return L.bpm_adam_step_groups(dt, TAB, 4, tb, *BUF, g, ngroups, 1.0, dev.get("scale"), dev.get("norm"), dev.get("steps"),
                                  dev.get("skipped"), 1, None)


def adam_sets(L, dt, nseg=3, total_off=0, **dev):
    sets = (_lib.AdamSet * 2)()
    for i, s in enumerate(sets):
        s.param, s.grad, s.exp_avg, s.exp_avg_sq, s.n = *(b + (i << 24) for b in BUF), 1 << 20
    tab = (_lib.AdamSeg * nseg)()
    blk = 0
    for i, s in enumerate(tab):
        s.off4, s.n4, s.blk0, s.group = 0 if i < 2 else 4096, 4096 if i < 2 else 1000, blk, _lib.adam_set_group(i & 1, i % 2)
        blk += L.bpm_adam_blocks(s.n4)
    g = (_lib.AdamGroup * 2)()
    for h in g:
        h.lr, h.beta1, h.beta2, h.eps, h.weight_decay, h.decoupled, h.step = 1e-3, 0.9, 0.999, 1e-8, 0.01, 0, 3
    return L.bpm_adam_step_sets(dt, TAB, tab, nseg, blk + total_off, TAB + 0x800, sets, 2, g, 2, 1.0, dev.get("scale"), dev.get("norm"),
                                dev.get("steps"), dev.get("skipped"), 1, None)


for _n in (4, 4 * 256, 4 * 256 * 4096, 4 * 256 * 4096 + 4, 6):
    case(f"adam_step n={_n}")(lambda L, n=_n: L.bpm_adam_step(*BUF, n, *HYPER, 3, 1.0, 1, None))
for _dn, _dt in DT.items():
    case(f"adam_step_table {_dn} 333 blocks")(lambda L, dt=_dt: L.bpm_adam_step_table(dt, TAB, 4, 333, *BUF, *HYPER, 3, 1.0, 1, None))
    case(f"adam_step_table_clip {_dn} 333 blocks")(lambda L, dt=_dt: L.bpm_adam_step_table_clip(dt, TAB, 4, 333, *BUF, *HYPER, 3, 1.0, SCALE, 1, None))
    case(f"adam_step_groups {_dn} host steps")(lambda L, dt=_dt: adam_groups(L, dt, 333))
    case(f"adam_step_groups {_dn} device steps")(lambda L, dt=_dt: adam_groups(L, dt, 333, scale=SCALE, norm=NORM, steps=STEPS, skipped=SKIPPED))
    case(f"adam_step_groups {_dn} skip counter only")(lambda L, dt=_dt: adam_groups(L, dt, 333, norm=NORM, skipped=SKIPPED))
    case(f"adam_step_groups {_dn} skip counter without a norm")(lambda L, dt=_dt: adam_groups(L, dt, 333, skipped=SKIPPED))
    case(f"adam_step_sets {_dn} host steps")(lambda L, dt=_dt: adam_sets(L, dt))
    case(f"adam_step_sets {_dn} device steps")(lambda L, dt=_dt: adam_sets(L, dt, scale=SCALE, norm=NORM, steps=STEPS, skipped=SKIPPED))
case("adam_step_table step 0")(lambda L: L.bpm_adam_step_table(BF, TAB, 4, 333, *BUF, *HYPER, 0, 1.0, 1, None))
case("adam_step_groups 17 groups")(lambda L: adam_groups(L, BF, 333, ngroups=17))
case("adam_step_groups steps 2 bytes off")(lambda L: adam_groups(L, BF, 333, steps=STEPS + 2))
case("adam_step_sets block count off by one")(lambda L: adam_sets(L, BF, total_off=1))


# ---------------------------------------------------------------------------------------------------------------------
# every grouped entry: BPM_MAX_GROUP problems are a launch, one more is BPM_ERR_ARG
# ---------------------------------------------------------------------------------------------------------------------
GROUPED = {
    "pack_rows_fwd": lambda L, n: pack_rows(L, BF, 2, 5, 7, n=n),
    "pack_rows_bwd": lambda L, n: pack_rows(L, BF, 2, 5, 7, n=n, bwd=True),
    "embed_pos_fwd": lambda L, n: embed(L, 5, 2, 8, n=n),
    "embed_pos_bwd": lambda L, n: embed(L, 5, 2, 8, n=n, bwd=True),
    "ln_fwd": lambda L, n: L.bpm_ln_fwd(BF, ln_problems(64, n=n), n, 64, 1e-5, None),
    "ln_bwd_ws": lambda L, n: ln_bwd(L, BF, 64, n=n),
    "kv_source_fwd": lambda L, n: kv_fwd(L, BF, 64, n=n),
    "kv_source_bwd": lambda L, n: kv_bwd(L, 64, n=n),
    "rows_cast": lambda L, n: cast(L, BF, 10, 64, n=n),
    "gelu_fwd": lambda L, n: gelu(L, BF, 10, 64, n=n),
    "gelu_bwd": lambda L, n: gelu(L, BF, 10, 64, n=n, bwd=True),
    "gmu2_fwd": lambda L, n: gmu(L, BF, 10, 64, n=n),
    "gmu2_bwd": lambda L, n: gmu(L, BF, 10, 64, n=n, bwd=True),
    "split_rows": lambda L, n: split(L, 10, 64, n=n),
    "add_n": lambda L, n: add_n(L, 64, n=n),
    "expand_heads": lambda L, n: expand(L, BF, 4, n=n),
}
for _name, _fn in GROUPED.items():
    case(f"{_name}: {MAX_GROUP} problems")(lambda L, fn=_fn: fn(L, MAX_GROUP))
    case(f"{_name}: {MAX_GROUP + 1} problems")(lambda L, fn=_fn: fn(L, MAX_GROUP + 1))
    case(f"{_name}: no problems")(lambda L, fn=_fn: fn(L, 0))
