"""Case table of the deterministic-mode row entries for the dry dispatch of the -DBPM_LAB build (the runner and the
address helpers are tests/rowops_cases.py's): bpm_ln_bwd_det, bpm_rows_cast_ws and bpm_unfold_grads_ws on both sides of
every threshold their choosers have, and their refusals beside the same call well formed.  A record is {"rc", "launches":
[[kernel, grid, block, last pointer argument], ...]}; profiles/deterministic_dispatch.json holds this tree's, written by
`python tests/deterministic_cases.py`, and tests/test_deterministic_cpu.py compares against it."""
import ctypes as C

from bpmult_amd import _lib
from rowops_cases import BASE, DT, Addr, ln_problems, run

CASES = {}
WS = BASE - (1 << 30)


def case(name):
    def deco(fn):
        assert name not in CASES, name
        CASES[name] = fn
        return fn
    return deco


def ln_det(L, dt, d, n=1, ws="fits", **kw):
    q = ln_problems(d, n=n, bwd=True, **kw)
    need = L.bpm_ln_bwd_det_ws_bytes(n, d)
    if ws == "short":                       # one float less than the launch's own blocks need (either route)
        scalar = d % 4 or d > 1024 or kw.get("share") or kw.get("dbeta_off") or kw.get("x_off")
        blocks = sum(min(256, max(1, (p.R + 3) // 4)) if scalar else min(64, max(1, (p.R + 7) // 8)) for p in q)
        need = (blocks * 3 * d + 64) * 4 - 4
    return L.bpm_ln_bwd_det(dt, q, n, d, 5, None if ws == "none" else WS, need, None)


for _dn, _dt in DT.items():
    for _d in (24, 50, 256, 768, 770, 1024, 1028, 1536, 2048, 2049):          # d % 4, and the vector kernels' reach (1024)
        case(f"ln_bwd_det {_dn} d={_d}")(lambda L, dt=_dt, d=_d: ln_det(L, dt, d))
    for _R in (4, 1024, 1028):                                                  # the scalar route's block cap (256 x 4 rows)
        case(f"ln_bwd_det {_dn} d=50 rows={_R} x 2")(lambda L, dt=_dt, R=_R: ln_det(L, dt, 50, n=2, R=R))
    case(f"ln_bwd_det {_dn} d=768 shared dgamma")(lambda L, dt=_dt: ln_det(L, dt, 768, n=2, share=True))
    case(f"ln_bwd_det {_dn} d=768 dbeta 4 bytes off")(lambda L, dt=_dt: ln_det(L, dt, 768, dbeta_off=4))
    case(f"ln_bwd_det {_dn} d=768 x 4 bytes off")(lambda L, dt=_dt: ln_det(L, dt, 768, x_off=4))
    case(f"ln_bwd_det {_dn} d=768 cast sums")(lambda L, dt=_dt: ln_det(L, dt, 768, cast_ldc=768, csum=True, drop_p=0.1))
    case(f"ln_bwd_det {_dn} d=1000 ldc=1024, cast sums")(lambda L, dt=_dt: ln_det(L, dt, 1000, cast_ldc=1024, csum=True))
    case(f"ln_bwd_det {_dn} d=50 no sums at all, no workspace")(lambda L, dt=_dt: ln_det(L, dt, 50, dgamma=False, ws="none"))
    for _d in (50, 768):
        case(f"ln_bwd_det {_dn} d={_d} null workspace")(lambda L, dt=_dt, d=_d: ln_det(L, dt, d, ws="none"))
        case(f"ln_bwd_det {_dn} d={_d} workspace one float short")(lambda L, dt=_dt, d=_d: ln_det(L, dt, d, n=2, ws="short"))
case("ln_bwd_det dtype 2")(lambda L: ln_det(L, 2, 768))


def cast_problems(shapes, ct=False, sums=True, share=False, lda=None, a_off=0):
    A = Addr()
    q = (_lib.CastProblem * len(shapes))()
    shared = A()
    for p, (R, Cn) in zip(q, shapes):
        p.a, p.lda, p.R, p.C = A(a_off), lda or Cn, R, Cn
        if ct:
            p.dst_ct, p.ldd = A(), (Cn + 31) // 32 * 32
        if sums:
            p.colsum = shared if share else A()
    return q


def cast_ws(L, dt, shapes, ws="fits", **kw):
    q = cast_problems(shapes, **kw)
    need = L.bpm_rows_cast_ws_bytes(q, len(q))
    return L.bpm_rows_cast_ws(dt, q, len(q), 5, None if ws == "none" else WS, 8 if ws == "short" else need, None)


for _dn, _dt in DT.items():
    for _C in (36, 37, 1024, 1028):                                             # colsum_kernel: C % 4 == 0 rows, at most 256 chunks
        for _R in (128, 129):                                                   # ... whose blocks are 128 rows (32 in rows_cast_kernel)
            case(f"rows_cast_ws {_dn} sums only {_R}x{_C}")(lambda L, dt=_dt, R=_R, Cn=_C: cast_ws(L, dt, [(R, Cn)]))
    case(f"rows_cast_ws {_dn} sums only 33x36, a 4 bytes off")(lambda L, dt=_dt: cast_ws(L, dt, [(33, 36)], a_off=4))
    case(f"rows_cast_ws {_dn} sums only 33x36 beside 33x37")(lambda L, dt=_dt: cast_ws(L, dt, [(33, 36), (33, 37)]))
    case(f"rows_cast_ws {_dn} dst_ct 33x36 and 129x1028")(lambda L, dt=_dt: cast_ws(L, dt, [(33, 36), (129, 1028)], ct=True))
    case(f"rows_cast_ws {_dn} shared colsum")(lambda L, dt=_dt: cast_ws(L, dt, [(129, 37), (33, 37)], share=True))
    case(f"rows_cast_ws {_dn} dst_ct, no sums")(lambda L, dt=_dt: cast_ws(L, dt, [(33, 36)], ct=True, sums=False))
    case(f"rows_cast_ws {_dn} null workspace")(lambda L, dt=_dt: cast_ws(L, dt, [(33, 36)], ws="none"))
    case(f"rows_cast_ws {_dn} workspace short")(lambda L, dt=_dt: cast_ws(L, dt, [(33, 36)], ws="short"))


def unfold_ws(L, ndesc, blocks, cols, ws="fits", table=BASE):
    need = L.bpm_unfold_grads_ws_bytes(ndesc, blocks, cols)
    return L.bpm_unfold_grads_ws(table, ndesc, blocks, 0, cols, None if ws == "none" else WS + (4 if ws == "off" else 0),
                                 need - 1 if ws == "short" else need, None)


case("unfold_grads_ws 6 descriptors of 96 blocks, 768 columns")(lambda L: unfold_ws(L, 6, 576, 768))
case("unfold_grads_ws 37 columns")(lambda L: unfold_ws(L, 2, 6, 37))
case("unfold_grads_ws null workspace")(lambda L: unfold_ws(L, 2, 6, 37, ws="none"))
case("unfold_grads_ws workspace one byte short")(lambda L: unfold_ws(L, 2, 6, 37, ws="short"))
case("unfold_grads_ws workspace 4 bytes off")(lambda L: unfold_ws(L, 2, 6, 37, ws="off"))
case("unfold_grads_ws null table")(lambda L: unfold_ws(L, 2, 6, 37, table=None))


def run_all(L):
    return {name: run(L, fn) for name, fn in CASES.items()}


if __name__ == "__main__":
    import json
    import os
    import sys
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.abspath(__file__)), ".."))
    L = _lib.bind_lab(_lib.load(_lib.build_lab()))
    rec = run_all(L)
    out = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..", "profiles", "deterministic_dispatch.json")
    with open(out, "w") as f:
        f.write("{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in rec.items()) + "\n}\n")
    print(f"{len(rec)} cases -> {out}")
