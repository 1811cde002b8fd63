#!/usr/bin/env python3
"""Micro-benchmark of the row kernels (LayerNorm fwd/bwd, rows_cast) at the model's shapes (MI355X only).

--streaming: the pure streaming kernels at the headline step's shapes (hidden 768) against ln_fwd in the same run --
unfold_grads over six descriptors of 1536 x 768, embed_pos forward / backward and ln_fwd over six problems of 4096 x 768;
--kv-source: the key / value sources of the six encoders of a level at the headline step's shape (twelve K / V problems
of 4096 x 768, bf16): the four launches embed_pos_fwd -> ln_fwd (hat) and ln_bwd (hat) -> embed_pos_bwd (+ add_n of the
two gradients) against bpm_kv_source_fwd / _bwd, with ln_fwd over the same twelve problems as the yardstick;
--json PATH writes {case: {"us", "GBps"}} (BPMULT_LIB selects the library, so two builds can alternate on one box)."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--d", type=int, default=300)
    ap.add_argument("--R", type=int, default=4096)
    ap.add_argument("--G", type=int, default=6)
    ap.add_argument("--iters", type=int, default=20)
    ap.add_argument("--streaming", action="store_true", help="only the streaming cases at hidden 768")
    ap.add_argument("--kv-source", action="store_true", help="only the key / value source cases at hidden 768")
    ap.add_argument("--json", default=None, help="write the results to this file")
    a = ap.parse_args()
    import bpmult_amd  # noqa: F401
    from bpmult_amd import ops
    from bpmult_amd.ops import BPM_BF16, pad32

    d, R, G = a.d, a.R, a.G
    ld = pad32(d)
    dev = "cuda"
    rn = lambda *s: torch.randn(*s, device=dev)

    def timeit(name, fn, nbytes):
        for _ in range(3):
            fn()
        torch.cuda.synchronize()
        ts = []
        for _ in range(a.iters):
            e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
            e0.record()
            fn()
            e1.record()
            e1.synchronize()
            ts.append(e0.elapsed_time(e1))
        ts.sort()
        med = ts[len(ts) // 2]
        print(f"{name:44s} {med * 1e3:8.1f} us  {nbytes / med / 1e6:8.1f} GB/s", flush=True)
        results[name] = {"us": round(med * 1e3, 2), "GBps": round(nbytes / med / 1e6, 1)}

    results = {}
    keep = []
    if a.streaming or a.kv_source:
        (kv_source_cases if a.kv_source else streaming_cases)(ops, timeit, a.G)
        if a.json:
            with open(a.json, "w") as f:
                json.dump(results, f, indent=1)
        return

    def ln_probs(n, gam=True, cast=False, add=True):
        ps = []
        for _ in range(n):
            x, g, mean, rstd, dy, addt, dx = rn(R, d), rn(d), rn(R), rn(R).abs(), rn(R, d), rn(R, d), rn(R, d)
            dg, db, cs = torch.zeros(d, device=dev), torch.zeros(d, device=dev), torch.zeros(d, device=dev)
            ct = torch.zeros(R, ld, device=dev, dtype=torch.bfloat16)
            keep.extend([x, g, mean, rstd, dy, addt, dx, dg, db, cs, ct])
            kw = dict(dgamma=dg, dbeta=db) if gam else {}
            if cast:
                kw.update(cast=ct, ldc=ld, cast_colsum=cs, drop_p=0.1, drop_site=3)
            ps.append(ops.ln_problem(x, g, None, mean, rstd, R, dy=dy, ldy=d, add=addt if add else None, dx=dx, **kw))
        return ops.array(ops.LnProblem, ps)

    base = R * d * 4 * 4
    for n in (G, 2 * G):
        for gam, cast in ((False, False), (True, False), (True, True)):
            arr = ln_probs(n, gam, cast)
            keep.append(arr)
            nb = n * (base + (R * ld * 2 if cast else 0))
            timeit(f"ln_bwd x{n} dgamma={int(gam)} cast={int(cast)}", lambda: ops.ln_bwd(arr, d, BPM_BF16, 5), nb)

    # ln fwd
    for n in (G, 2 * G):
        ps = []
        for _ in range(n):
            x, g, b, mean, rstd = rn(R, d), rn(d), rn(d), rn(R), rn(R)
            out = torch.zeros(R, ld, device=dev, dtype=torch.bfloat16)
            keep.extend([x, g, b, mean, rstd, out])
            ps.append(ops.ln_problem(x, g, b, mean, rstd, R, out=out, ldo=ld))
        arr2 = ops.array(ops.LnProblem, ps)
        keep.append(arr2)
        timeit(f"ln_fwd x{n}", lambda: ops.ln_fwd(BPM_BF16, arr2, d), n * (R * d * 4 + R * ld * 2))

    # colsum of CT rows (in_proj bias gradients)
    ps = []
    for _ in range(3 * G):
        src = torch.randn(R, ld, device=dev).to(torch.bfloat16)
        cs = torch.zeros(d, device=dev)
        keep.extend([src, cs])
        ps.append(ops.cast_problem(src, ld, R, d, a_is_ct=True, colsum=cs))
    arr3 = ops.array(ops.CastProblem, ps)
    timeit(f"rows_cast colsum-only x{3 * G}", lambda: ops.rows_cast(BPM_BF16, arr3, 5), 3 * G * R * ld * 2)
    # f32 -> CT cast with dropout + colsum
    ps = []
    for _ in range(G):
        src, cs = rn(R, d), torch.zeros(d, device=dev)
        dst = torch.zeros(R, ld, device=dev, dtype=torch.bfloat16)
        keep.extend([src, cs, dst])
        ps.append(ops.cast_problem(src, d, R, d, dst_ct=dst, ldd=ld, colsum=cs, drop_p=0.1, drop_site=4))
    arr4 = ops.array(ops.CastProblem, ps)
    timeit(f"rows_cast f32->CT drop colsum x{G}", lambda: ops.rows_cast(BPM_BF16, arr4, 5), G * (R * d * 4 + R * ld * 2))


def streaming_cases(ops, timeit, G, R=4096, d=768):
    """Bytes are algorithmic: every matrix once per direction it moves in; the [d] vectors and the cached position
    table are left out."""
    from bpmult_amd import _lib
    from bpmult_amd.ops import BPM_BF16, pad32
    dev = "cuda"
    rn = lambda *s: torch.randn(*s, device=dev)
    keep = []

    # unfold_grads: in_proj rows [d, 3d) of one layer of six encoders
    rows, descs = 2 * d, []
    for k in range(G):
        t = [rn(rows, d), rn(rows), rn(rows, d), rn(d), rn(d), rn(rows, d), rn(rows), rn(d), rn(d)]
        keep.append(t)
        ud = _lib.UnfoldDesc()
        (ud.dWf, ud.dbf, ud.W, ud.gamma, ud.beta, ud.dW, ud.dbias, ud.dgamma, ud.dbeta) = (x.data_ptr() for x in t)
        ud.rows, ud.cols, ud.ldw, ud.blk0 = rows, d, d, k * ((rows + 15) // 16)
        descs.append(ud)
    tab, nblk = ops.device_table(descs), G * ((rows + 15) // 16)
    for store in (0, 1):
        timeit(f"unfold_grads x{G} {rows}x{d} store_dw={store}", lambda: ops.unfold_grads(tab, G, nblk, store_dw=bool(store)),
               G * rows * d * 4 * (3 if store else 4))
        # deterministic mode: dgamma / dbeta through per-block partial rows instead of float atomics
        timeit(f"unfold_grads_ws x{G} {rows}x{d} store_dw={store}", lambda: ops.unfold_grads_ws(tab, G, nblk, d, store_dw=bool(store)),
               G * rows * d * 4 * (3 if store else 4))

    # embed_pos: T*B = R rows
    T, B = R // 8, 8
    table = rn(T + 2, d)
    x, out = [rn(T, B, d) for _ in range(G)], [rn(T, B, d) for _ in range(G)]
    for p in (0.0, 0.25):
        fw = ops.array(ops.EmbedProblem, [ops.embed_problem(x[k], out[k], T, B, drop_p=p, drop_site=k) for k in range(G)])
        timeit(f"embed_pos_fwd x{G} {R}x{d} drop={p}", lambda: ops.embed_pos_fwd(fw, table, d, d ** 0.5, seed=1), G * R * d * 4 * 2)
        for acc in (0, 1):
            bw = ops.array(ops.EmbedProblem, [ops.embed_problem(x[k], out[k], T, B, accumulate=bool(acc), drop_p=p, drop_site=k)
                                              for k in range(G)])
            timeit(f"embed_pos_bwd x{G} {R}x{d} drop={p} accumulate={acc}", lambda: ops.embed_pos_bwd(bw, d, d ** 0.5, seed=1),
                   G * R * d * 4 * (3 if acc else 2))

    # ln_fwd: the rate the same file reaches on the same rows
    ld, ps = pad32(d), []
    for _ in range(G):
        t = [rn(R, d), rn(d), rn(d), rn(R), rn(R), torch.zeros(R, ld, device=dev, dtype=torch.bfloat16)]
        keep.append(t)
        ps.append(ops.ln_problem(t[0], t[1], t[2], t[3], t[4], R, out=t[5], ldo=ld))
    arr = ops.array(ops.LnProblem, ps)
    timeit(f"ln_fwd x{G} {R}x{d}", lambda: ops.ln_fwd(BPM_BF16, arr, d), G * (R * d * 4 + R * ld * 2))


def kv_source_cases(ops, timeit, G, S=512, B=8, d=768):
    """Bytes are algorithmic, in units of one fp32 [S B, d] tensor (Rb): the two-kernel route moves 7 Rb forward (source
    twice, ke / ve written and read, khat / vhat as bf16) and 10 Rb backward (+ 2 Rb read and 1 Rb written by add_n); the
    fused launches 2 Rb forward and 4 Rb backward (source, Gk, Gv, one summed gradient; 5 Rb with separate gradients)."""
    from bpmult_amd.ops import BPM_BF16, pad32
    dev = "cuda"
    rn = lambda *s: torch.randn(*s, device=dev)
    R, ld, scale, p = S * B, pad32(d), d ** 0.5, 0.25
    Rb = R * d * 4
    table = rn(S + 2, d)
    ones, zeros = torch.ones(d, device=dev), torch.zeros(d, device=dev)
    z = lambda *s, dt=torch.float32: torch.zeros(*s, device=dev, dtype=dt)
    keep, emb, hat, hat_b, emb_b, add, kv, kvm, yard = [], [], [], [], [], [], [], [], []
    for k in range(G):
        x, gk, gv = rn(S, B, d), rn(R, d), rn(R, d)
        t = dict(ke=z(R, d), ve=z(R, d), dke=z(R, d), dve=z(R, d), khat=z(R, ld, dt=torch.bfloat16), vhat=z(R, ld, dt=torch.bfloat16),
                 dxk=z(S, B, d), dxv=z(S, B, d), dx=z(S, B, d), st=[z(R) for _ in range(4)])
        keep += [x, gk, gv, t]
        st = t["st"]
        emb += [ops.embed_problem(x, t["ke"], S, B, drop_p=p, drop_site=2 * k), ops.embed_problem(x, t["ve"], S, B, drop_p=p, drop_site=2 * k + 1)]
        hat += [ops.ln_problem(t["ke"], ones, zeros, st[0], st[1], R, out=t["khat"], ldo=ld),
                ops.ln_problem(t["ve"], ones, zeros, st[2], st[3], R, out=t["vhat"], ldo=ld)]
        hat_b += [ops.ln_problem(t["ke"], ones, None, st[0], st[1], R, dy=gk, ldy=d, dx=t["dke"]),
                  ops.ln_problem(t["ve"], ones, None, st[2], st[3], R, dy=gv, ldy=d, dx=t["dve"])]
        emb_b += [ops.embed_problem(t["dke"], t["dxk"], S, B, drop_p=p, drop_site=2 * k),
                  ops.embed_problem(t["dve"], t["dxv"], S, B, drop_p=p, drop_site=2 * k + 1)]
        add.append(ops.addn_problem(t["dx"], [t["dxk"], t["dxv"]]))
        kw = dict(khat=t["khat"], vhat=t["vhat"], ld=ld, stats_k=(st[0], st[1]), stats_v=(st[2], st[3]), gk=gk, gv=gv, drop_p=p,
                  drop_site_k=2 * k, drop_site_v=2 * k + 1)
        kv.append(ops.kv_source_problem(x, x, S, B, dxk=t["dxk"], dxv=t["dxv"], **kw))
        kvm.append(ops.kv_source_problem(x, x, S, B, dxk=t["dx"], dxv=None, **kw))
    emb, emb_b = ops.array(ops.EmbedProblem, emb), ops.array(ops.EmbedProblem, emb_b)
    hat, hat_b = ops.array(ops.LnProblem, hat), ops.array(ops.LnProblem, hat_b)
    add = ops.array(ops._lib.AddnProblem, add)
    kv, kvm = ops.array(ops.KvSourceProblem, kv), ops.array(ops.KvSourceProblem, kvm)
    n = 2 * G
    timeit(f"embed_pos_fwd x{n} {R}x{d}", lambda: ops.embed_pos_fwd(emb, table, d, scale, seed=1), G * 4 * Rb)
    timeit(f"ln_fwd (hat) x{n}", lambda: ops.ln_fwd(BPM_BF16, hat, d), G * 3 * Rb)
    timeit(f"ln_bwd (hat) x{n}", lambda: ops.ln_bwd(hat_b, d, BPM_BF16, 1), G * 6 * Rb)
    timeit(f"embed_pos_bwd x{n}", lambda: ops.embed_pos_bwd(emb_b, d, scale, seed=1), G * 4 * Rb)
    timeit(f"add_n x{G} (dxk + dxv)", lambda: ops.add_n(add), G * 3 * Rb)
    timeit(f"kv_source_fwd x{G}", lambda: ops.kv_source_fwd(BPM_BF16, kv, table, d, scale, seed=1), G * 2 * Rb)
    timeit(f"kv_source_bwd x{G} separate", lambda: ops.kv_source_bwd(kv, table, d, scale, seed=1), G * 5 * Rb)
    timeit(f"kv_source_bwd x{G} merged", lambda: ops.kv_source_bwd(kvm, table, d, scale, seed=1), G * 4 * Rb)
    for _ in range(n):
        t = [rn(R, d), rn(d), rn(d), rn(R), rn(R), torch.zeros(R, ld, device=dev, dtype=torch.bfloat16)]
        keep.append(t)
        yard.append(ops.ln_problem(t[0], t[1], t[2], t[3], t[4], R, out=t[5], ldo=ld))
    yard = ops.array(ops.LnProblem, yard)
    timeit(f"ln_fwd x{n} {R}x{d} (yardstick)", lambda: ops.ln_fwd(BPM_BF16, yard, d), n * (Rb + R * ld * 2))


if __name__ == "__main__":
    main()
