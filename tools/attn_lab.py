#!/usr/bin/env python3
"""Attention kernel lab (MI355X only): the three attention launches of one encoder layer at the headline workload's
shapes -- six lock-stepped encoders, B=8, H=12 heads of 64, T=S=512, future mask, attention dropout .1 on two of the six
(README rates) -- timed stand-alone with HIP events (median of --iters launches, random data).

  python tools/attn_lab.py [--H 12 --dh 64 --T 512 --S 512 --B 8 --G 6 --no-mask --drop 0.1]
  rocprofv3 --pmc SQ_WAVES SQ_BUSY_CYCLES ... -- python3 tools/attn_lab.py --iters 3     (counters per kernel)

--maps: also the head-averaged attention-map launch (bpm_attn_maps: one problem per encoder, fp32 [B, T, S] out) beside the
forward launch of the same shapes in the same run -- it does one of the forward's two products and the same exponentials,
so the forward time is its yardstick.  Shapes on record: the default (headline), the kernel point
`--H 6 --dh 128 --T 50 --S 50 --B 64`, and head_dim 256 `--H 6 --dh 256`.
--maps --per-head: the per-head launch too (bpm_attn_head_maps: fp32 [B, H, T, S] out, H times the bytes), alternating with
the averaged launch and the forward in the same three rounds; reports the bytes written and the achieved store rate of both
(profiles/head_maps_lab.json holds the three shapes above).

--amask: also the additive-mask entries (bpm_attn_fwd_amask / _bwd_dq_amask / _bwd_dkv_amask) at the same shapes in the same
run, twice: with an all-zeros [T, S] mask on top of the same mask_off rule (the unmasked launches' arithmetic plus the mask
reads: the cost of the mask path), and with the future mask itself as a -inf tensor and no mask_off rule (what a caller
pays who states a structured mask as a tensor: no tile is skipped).  And the learned-bias launches (`dbias`): with an all-zeros
mask and the same rule, for one encoder and for all G in one launch, bpm_attn_bwd_dbias in both forms (shared [T, S]: the
head sums are split over workgroups when the launch has fewer than 256 tiles; per head [H, T, S]) beside the dQ and dK / dV
launches of the same problems, and forward / dQ / dK / dV with H mask images through the head stride against one image.

--kamask: the combined-mask entries (bpm_attn_fwd_kamask / _bwd_dq_kamask / _bwd_dkv_kamask) beside the two families they are
made of, on the same inputs in the same run, the three alternating in each of three rounds (median round on record): the
*_hmask entries with an all-zeros image, the *_kmask entries and the *_kamask entries with an all-ones byte mask, and the
latter two again with the last third of every sample's keys padded.  --f32 times everything in float32.

--bmask: the per-sample entries (bpm_attn_fwd_bmask / _bwd_dq_bmask / _bwd_dkv_bmask) beside the *_hmask entries at the same
shape in the same run, alternating in three rounds: all-zeros images as [H,T,S] through *_hmask, the same through *_bmask at
batch stride 0, [B,1,T,S] and [B,H,T,S] (one set of images per encoder).  Also prints the image bytes every pass reads,
from the shapes: at T = S = 512, B = 8, H = 12 a [B,H,T,S] image is 100.7 MB per encoder, the shared [T,S] one 1 MB.

Algorithmic FLOPs per visible (query, key) pair and head: forward 4 dh, dQ pass 6 dh (S, dP, dQ), dK/dV pass 8 dh."""
import argparse
import json
import os
import sys

import torch

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bpmult_amd  # noqa: E402,F401
from bpmult_amd import ops  # noqa: E402
from bpmult_amd.engine import dhp_for  # noqa: E402
from bpmult_amd.ops import BPM_BF16  # noqa: E402


BF16_PEAK_TF = 2500.0     # MI355X dense bf16 MFMA peak (spec)


def _time(fn, iters):
    for _ in range(2):
        fn()
    torch.cuda.synchronize()
    ts = []
    for _ in range(iters):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        fn()
        e1.record()
        e1.synchronize()
        ts.append(e0.elapsed_time(e1))
    ts.sort()
    return ts[len(ts) // 2] * 1e3


def main():
    ap = argparse.ArgumentParser()
    for k, v in (("H", 12), ("dh", 64), ("T", 512), ("S", 512), ("B", 8), ("G", 6), ("iters", 20)):
        ap.add_argument("--" + k, type=int, default=v)
    ap.add_argument("--drop", type=float, default=0.1)
    ap.add_argument("--drop-encoders", type=int, default=2, help="how many of the G encoders have attention dropout")
    ap.add_argument("--no-mask", action="store_true")
    ap.add_argument("--maps", action="store_true", help="also time bpm_attn_maps at the same shapes (after the forward has written LSE)")
    ap.add_argument("--per-head", action="store_true", help="with --maps: also time bpm_attn_head_maps on the same buffers")
    ap.add_argument("--amask", action="store_true", help="also time the *_amask entries (all-zeros mask; the future mask as a tensor)")
    ap.add_argument("--kamask", action="store_true", help="also time the *_kamask entries beside the *_kmask and *_hmask entries")
    ap.add_argument("--bmask", action="store_true", help="also time the *_bmask entries (one all-zeros image per sample) beside the *_hmask entries")
    ap.add_argument("--f32", action="store_true", help="float32 instead of bfloat16")
    ap.add_argument("--pair", type=int, default=-1, help="tuning hook: bit k = kernel k (fwd, dQ, dK/dV) takes two blocks per workgroup")
    a = ap.parse_args()
    dev, ct = "cuda", torch.float32 if a.f32 else torch.bfloat16
    DT = ops.BPM_F32 if a.f32 else BPM_BF16
    if a.pair >= 0:
        from bpmult_amd import _lib
        _lib.check(_lib.lab_library().__enter__().bpm_debug_attn_pair(a.pair), "bpm_debug_attn_pair")   # -DBPM_LAB build only
    B, H, T, S, dh, G = a.B, a.H, a.T, a.S, a.dh, a.G
    dhp = dhp_for(dh)
    d = H * dh
    off = (1 << 30) if a.no_mask else 1 + abs(S - T)
    g = torch.Generator().manual_seed(3)
    rb = lambda *s: (torch.randn(*s, generator=g) * 0.5).to(ct).to(dev)
    keep, probs = [], []
    for e in range(G):
        t = dict(q=rb(B, H, T, dhp), k=rb(B, H, S, dhp), v=rb(B, H, S, dhp), do=rb(B, H, T, dhp),
                 o=torch.zeros(T * B, d, device=dev, dtype=ct), lse=torch.zeros(B, H, T, device=dev),
                 delta=torch.zeros(B, H, T, device=dev), dq=torch.zeros(T * B, d, device=dev, dtype=ct),
                 dk=torch.zeros(S * B, d, device=dev, dtype=ct), dv=torch.zeros(S * B, d, device=dev, dtype=ct))
        keep.append(t)
        probs.append(ops.attn_problem(t["q"], t["k"], t["v"], t["o"], d, t["lse"], B, H, T, S, dh, dhp, off, dO=t["do"], delta=t["delta"],
                                      dQ=t["dq"], lddq=d, dK=t["dk"], lddk=d, dV=t["dv"], lddv=d, dq_scale=dh ** -0.5,
                                      drop_p=a.drop if e < a.drop_encoders else 0.0, drop_site=9 + 16 * e))
    arr = ops.array(ops.AttnProblem, probs)
    pairs = sum(min(S, t + off) for t in range(T)) * B * H * G
    res = {"shape": dict(B=B, H=H, T=T, S=S, head_dim=dh, encoders=G, mask=not a.no_mask, drop=a.drop, drop_encoders=a.drop_encoders,
                         dtype="f32" if a.f32 else "bf16")}
    for name, fn, fl in (("fwd", ops.attn_fwd, 4), ("bwd_dq", ops.attn_bwd_dq, 6), ("bwd_dkv", ops.attn_bwd_dkv, 8)):
        us = _time(lambda: fn(DT, arr, 5), a.iters)
        tf = fl * dh * pairs / us / 1e6
        res[name] = {"us": round(us, 1), "tflops": round(tf, 1), "bf16_peak_frac": round(tf / BF16_PEAK_TF, 3)}
    if a.amask:
        ldm, ldt = (S + 3) // 4 * 4, (T + 3) // 4 * 4
        zeros = (torch.zeros(T, ldm, device=dev), torch.zeros(S, ldt, device=dev))
        hidden = (torch.arange(S)[None, :] - torch.arange(T)[:, None]) >= 1 + abs(S - T)
        fm, ft = torch.zeros(T, ldm), torch.zeros(S, ldt)
        fm[:, :S][hidden] = float("-inf")
        ft[:, :T][hidden.t()] = float("-inf")
        fut = (fm.to(dev), ft.to(dev))
        free = ops.array(ops.AttnProblem, probs)          # the same problems without the mask_off rule
        for p in free:
            p.mask_off = 0
        for tag, (m, mt), parr in (("amask_zeros", zeros, arr), ("amask_future_tensor", fut, free)):
            am = ops.attn_amasks([(m, ldm, mt, ldt)] * G)
            res[tag] = {}
            for name, fn in (("fwd", ops.attn_fwd_amask), ("bwd_dq", ops.attn_bwd_dq_amask), ("bwd_dkv", ops.attn_bwd_dkv_amask)):
                us = _time(lambda: fn(DT, parr, am, 5), a.iters)
                res[tag][name] = {"us": round(us, 1), "over_unmasked": round(us / res[name]["us"], 3)}
        # the learned-bias launches: all-zeros images, one per head through the head stride, and the bias gradient
        zh = (torch.zeros(H, T, ldm, device=dev), torch.zeros(H, S, ldt, device=dev))
        res["dbias"] = {}
        for n in sorted({1, G}):
            sub = ops.array(ops.AttnProblem, probs[:n])
            am0 = ops.attn_amasks([(zeros[0], ldm, zeros[1], ldt)] * n)
            amh = ops.attn_amasks([(zh[0], ldm, zh[1], ldt, T * ldm, S * ldt)] * n)
            r = res["dbias"][f"{n}_problems"] = {}
            for name, fn in (("fwd", ops.attn_fwd_amask), ("bwd_dq", ops.attn_bwd_dq_amask), ("bwd_dkv", ops.attn_bwd_dkv_amask)):
                u0, uh = _time(lambda: fn(DT, sub, am0, 5), a.iters), _time(lambda: fn(DT, sub, amh, 5), a.iters)
                r[name] = {"us_stride0": round(u0, 1), "us_head_stride": round(uh, 1), "head_over_stride0": round(uh / u0, 3)}
            tiles = ((T + 63) // 64) * ((S + 63) // 64)
            for form, nimg, am in (("shared", 1, am0), ("per_head", H, amh)):
                g = [torch.empty(nimg, T, ldm, device=dev) for _ in range(n)]
                outs = ops.attn_dbias([(x, ldm, T * ldm if nimg > 1 else 0) for x in g])
                nws = ops.attn_dbias_ws_bytes(sub, outs)
                ws = torch.empty(nws // 4, device=dev) if nws else None
                us = _time(lambda: ops.attn_bwd_dbias(DT, sub, am, outs, 5, ws=ws), a.iters)
                splits = nws // (n * nimg * T * ldm * 4) if nws else 1
                r["dbias_" + form] = {"us": round(us, 1), "over_dq": round(us / r["bwd_dq"]["us_head_stride" if nimg > 1 else "us_stride0"], 3),
                                      "workgroups": n * nimg * tiles * splits, "splits_per_tile": splits, "workspace_mbytes": round(nws / 1e6, 2)}
    if a.kamask:
        ldm, ldt = (S + 3) // 4 * 4, (T + 3) // 4 * 4
        am = ops.attn_amasks([(torch.zeros(T, ldm, device=dev), ldm, torch.zeros(S, ldt, device=dev), ldt)] * G)
        ones = torch.ones(B, S, dtype=torch.uint8, device=dev)
        third = ones.clone()
        third[:, S - S // 3:] = 0
        res["kamask"] = {}
        for tag, kb in (("all_ones", ones), ("third_padded", third)):
            km = ops.attn_kmasks([(kb, S)] * G)
            r = res["kamask"][tag] = {}
            for name in ("fwd", "bwd_dq", "bwd_dkv"):
                fh, fk, fka = (getattr(ops, f"attn_{name}_{fam}") for fam in ("amask", "kmask", "kamask"))
                rounds = []
                for _ in range(3):
                    rounds.append((_time(lambda: fh(DT, arr, am, 5), a.iters), _time(lambda: fk(DT, arr, km, 5), a.iters),
                                   _time(lambda: fka(DT, arr, km, am, 5), a.iters)))
                uh, uk, uka = (sorted(x[i] for x in rounds)[1] for i in range(3))
                r[name] = {"hmask_us": round(uh, 1), "kmask_us": round(uk, 1), "kamask_us": round(uka, 1),
                           "kamask_over_hmask": round(uka / uh, 3), "kamask_over_kmask": round(uka / uk, 3),
                           "rounds_hmask_kmask_kamask_us": [[round(x, 1) for x in y] for y in rounds]}
    if a.bmask:
        # per-sample images (the *_bmask entries) beside the shared-image entries at the same shape: all-zeros images, one
        # set per encoder (nothing is shared between the problems of a launch), three rounds, the middle one reported
        ldm, ldt = (S + 3) // 4 * 4, (T + 3) // 4 * 4

        def images(Bm, Hm, per_sample):
            out = []
            for _ in range(G):
                m, mt = torch.zeros(Bm, Hm, T, ldm, device=dev), torch.zeros(Bm, Hm, S, ldt, device=dev)
                hs, hst = (T * ldm, S * ldt) if Hm > 1 else (0, 0)
                bs, bst = (Hm * T * ldm, Hm * S * ldt) if Bm > 1 else (0, 0)
                out.append((m, ldm, mt, ldt, hs, hst) + ((bs, bst) if per_sample else ()))
            return ops.attn_amasks(out), out

        forms = (("hmask_HTS", images(1, H, False), H), ("bmask_HTS_stride0", images(1, H, True), H),
                 ("bmask_B1TS", images(B, 1, True), B), ("bmask_BHTS", images(B, H, True), B * H))
        res["bmask"] = {"image_mbytes_per_pass": {tag: round(G * n * T * S * 4 / 1e6, 1) for tag, _, n in forms}}
        for name, fn in (("fwd", ops.attn_fwd_amask), ("bwd_dq", ops.attn_bwd_dq_amask), ("bwd_dkv", ops.attn_bwd_dkv_amask)):
            rounds = [[_time(lambda: fn(DT, arr, am, 5), a.iters) for _, (am, _), _ in forms] for _ in range(3)]
            mid = [sorted(r[i] for r in rounds)[1] for i in range(len(forms))]
            res["bmask"][name] = {tag + "_us": round(u, 1) for (tag, _, _), u in zip(forms, mid)}
            res["bmask"][name].update({tag + "_over_hmask": round(u / mid[0], 3) for (tag, _, _), u in list(zip(forms, mid))[1:]})
            res["bmask"][name]["rounds_us"] = [[round(x, 1) for x in r] for r in rounds]
    if a.maps:
        # LSE of the last forward launch above is in place; maps and forward alternate in one timing loop each, three rounds
        wts = [torch.empty(B, T, S, device=dev) for _ in range(G)]
        mp = [ops.attn_map_problem(t["q"], t["k"], t["lse"], w, S, B, H, T, S, dh, dhp, off) for t, w in zip(keep, wts)]
        marr = ops.array(ops.AttnMapProblem, mp)
        ops.attn_fwd(DT, arr, 5)
        rounds = []
        if a.per_head:
            hts = [torch.empty(B, H, T, S, device=dev) for _ in range(G)]
            harr = ops.array(ops.AttnHeadMapProblem, [ops.attn_head_map_problem(t["q"], t["k"], t["lse"], w, S, B, H, T, S, dh, dhp, off)
                                                      for t, w in zip(keep, hts)])
        for _ in range(3):
            rounds.append((_time(lambda: ops.attn_fwd(DT, arr, 5), a.iters), _time(lambda: ops.attn_maps(DT, marr), a.iters))
                          + ((_time(lambda: ops.attn_head_maps(DT, harr), a.iters),) if a.per_head else ()))
        f_us, m_us = sorted(r[0] for r in rounds)[1], sorted(r[1] for r in rounds)[1]
        out_bytes = G * B * T * S * 4
        in_bytes = G * B * H * ((T + S) * dhp * 2 + T * 4)
        rowsum = float((wts[0].double().sum(-1) - 1.0).abs().max())
        res["maps"] = {"us": round(m_us, 1), "fwd_us_same_run": round(f_us, 1), "maps_over_fwd": round(m_us / f_us, 3),
                       ("rounds_fwd_maps_head_us" if a.per_head else "rounds_fwd_maps_us"): [[round(x, 1) for x in r] for r in rounds],
                       "out_mbytes": round(out_bytes / 1e6, 1), "hbm_gbytes_per_s": round((out_bytes + in_bytes) / m_us / 1e3, 1),
                       "tflops": round(2 * dh * B * H * G * T * S / m_us / 1e6, 1), "max_row_sum_error": rowsum,
                       "store_gbytes_per_s": round(out_bytes / m_us / 1e3, 1)}
        if a.per_head:
            h_us = sorted(r[2] for r in rounds)[1]
            mean = torch.zeros_like(wts[0])
            for h in range(H):
                mean += hts[0][:, h]
            mean *= torch.ones((), device=dev) / H
            res["head_maps"] = {"us": round(h_us, 1), "maps_us_same_run": round(m_us, 1), "head_over_maps": round(h_us / m_us, 3),
                                "head_over_fwd": round(h_us / f_us, 3), "out_mbytes": round(H * out_bytes / 1e6, 1),
                                "store_gbytes_per_s": round(H * out_bytes / h_us / 1e3, 1),
                                "hbm_gbytes_per_s": round((H * out_bytes + in_bytes) / h_us / 1e3, 1),
                                "tflops": round(2 * dh * B * H * G * T * S / h_us / 1e6, 1),
                                "max_row_sum_error": float((hts[0].double().sum(-1) - 1.0).abs().max()),
                                "head_sum_bit_equal_to_maps": bool(torch.equal(mean, wts[0]))}
    print(json.dumps(res))


if __name__ == "__main__":
    main()
