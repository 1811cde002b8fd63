"""Time what a sharded evaluation adds on each rank: bpm_eval_pack of its shard and bpm_eval_merge of all images, beside
the replicated bpm_eval_finalize they feed (profiles/eval_shard.json).

One GPU plays every rank: N = 8192 rows of C = 23 classes in batches of 8 (the size at which DESIGN.md section 5 times
finalize), dealt to W = 8 shards of 1024 rows.  Device events around `--inner` back-to-back (pack, merge) pairs, divided
by their number, `--repeats` times after a warm-up; finalize alone the same way.  The collective between pack and merge is
not timed here (no box with two GPUs): its message is the image, whose bytes are recorded.  A record, not a gate.

    python tools/eval_shard_time.py [--repeats 5] [--inner 200]      # on an MI355X, after build()
"""
import argparse
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
if ROOT not in sys.path:
    sys.path.insert(0, ROOT)

import torch  # noqa: E402

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import metrics, ops  # noqa: E402

N, C, W, BS = 8192, 23, 8, 8


def timed(fn, inner, repeats):
    out = []
    for _ in range(repeats + 1):                    # the first window is the warm-up
        a, b = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        a.record()
        for _ in range(inner):
            fn()
        b.record()
        torch.cuda.synchronize()
        out.append(a.elapsed_time(b) / inner)
    return sorted(out[1:])


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--repeats", type=int, default=5)
    ap.add_argument("--inner", type=int, default=200)
    ap.add_argument("--out", default=os.path.join(ROOT, "profiles", "eval_shard.json"))
    a = ap.parse_args()
    if not torch.cuda.is_available():
        raise SystemExit("eval_shard_time: needs an MI355X; there is nothing to time on a CPU")
    g = torch.Generator().manual_seed(3)
    x = (torch.randint(-24, 25, (N, C), generator=g) / 8).cuda()
    y = (torch.rand(N, C, generator=g) < 0.3).float().cuda()
    per = N // W
    shards = []
    for r in range(W):
        ev = metrics.Evaluator("multilabel", C, per, device="cuda")
        for lo in range(r * per, (r + 1) * per, BS):
            ev.update(x[lo:lo + BS], y[lo:lo + BS], torch.tensor(0.5, device="cuda"))
        shards.append(ev)
    nb = per // BS
    images = torch.stack([ev.pack(per, nb) for ev in shards])
    dest = metrics.Evaluator("multilabel", C, N, device="cuda")
    slot = torch.empty_like(images[0])
    rows, batches = [per] * W, [nb] * W

    def pair():
        shards[0].pack(per, nb, out=slot)
        dest.merge(images, rows, batches)

    t_pair = timed(pair, a.inner, a.repeats)
    t_fin = timed(lambda: ops.eval_finalize(dest._desc, dest.n, dest.nlosses), 5, a.repeats)
    ms = lambda v: {"median": round(v[len(v) // 2], 4), "min": round(v[0], 4), "max": round(v[-1], 4)}      # noqa: E731
    rec = {"device": torch.cuda.get_device_name(0), "N": N, "C": C, "world": W, "batch": BS,
           "image_bytes_per_rank": images.shape[1] * 4, "exchange_buffer_bytes": images.numel() * 4,
           "pack_plus_merge_ms": ms(t_pair), "finalize_ms": ms(t_fin), "repeats": a.repeats, "inner": a.inner,
           "how": "device events around `inner` back-to-back (pack, merge) pairs on one stream, host launch cost included; "
                  "finalize: 5 back-to-back calls per window"}
    with open(a.out, "w") as f:
        json.dump(rec, f, indent=1)
        f.write("\n")
    print(json.dumps(rec))


if __name__ == "__main__":
    main()
