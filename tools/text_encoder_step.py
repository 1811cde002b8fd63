#!/usr/bin/env python3
"""Forward + backward of the text encoder ALONE at the bert-base shape (12 layers, d = 768, 12 heads, intermediate 3072,
L = 512, B = 8, HF dropout defaults 0.1, train mode, randomly initialised weights -- nothing is downloaded), four ways:

  hf_f32     HF BertModel in fp32, no autocast       (the reference's setting, mmtr.py:144-158)
  hf_bf16    HF BertModel under torch.autocast(bf16)
  hip_f32    text_encoder="hip", precision f32       (embeddings on torch, the layer stack on the HIP path)
  hip_bf16   text_encoder="hip", precision bf16

`--embeddings hip` runs the two hip modes with text_embeddings="hip" (ids -> hidden state -> backward as one autograd node,
models/bert.py:run_encoder) and records them as hip_f32_hip_embeddings / hip_bf16_hip_embeddings; `--modes` selects a subset.
With `--out`, modes that were not run keep the figures the file already holds.

  python tools/text_encoder_step.py [--steps 40 --warmup 5 --repeats 3 --out profiles/text_encoder_step.json]
  python tools/text_encoder_step.py --modes hip_bf16 --embeddings hip --out profiles/text_encoder_step.json

Every mode runs in a child process of its own under `timeout` (a hung or faulted mode ends the whole measurement: nothing
more is started on the device).  In the child: `--warmup` untimed steps, then `--repeats` windows of `--steps` steps, each
between two device synchronisations and timed with events on the current stream; the median window and the spread
(max - min) / median are reported.  A step is embeddings + layers forward, a loss that weights every position, and the
backward down to the word embeddings.  No optimizer runs, so the HIP modes re-pack their weight shadows explicitly in every
step (what an optimizer step would make them do; HF's autocast casts its weights inside every step too).  The default
windows are 40 steps (0.4 - 1.2 s each).  All positions are real tokens (full-length mask: the most work a batch can be).
`--optimizer` measures the whole training step instead: forward + backward + `FusedAdam.step()` of a model with this text
encoder (hip_bf16, HIP embeddings) in front of a toy trunk (hidden 24, one layer), `args.text_params = "torch"` against
`"flat"`, alternated `--rounds` times in one call, one child process per run.  Per run: the median window and spread as
above, the bytes the caching allocator handed out per step (`torch.cuda.memory_stats`, allocated_bytes.all.allocated), and
the device kernels of ONE optimizer step counted with torch.profiler after the timing.  Written to `--out`
(profiles/text_params_step.json):

  python tools/text_encoder_step.py --optimizer [--rounds 2] --out profiles/text_params_step.json

Algorithmic flops per step (forward + backward = 3x forward; per layer 8 L d^2 for q / k / v / out, 4 L^2 d for the two
attention products, 4 L d I for the FFN): printed as TFLOP/s next to each time -- a whole-step rate, not a kernel's."""
import argparse
import json
import os
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)

SHAPE = dict(layers=12, d=768, heads=12, inter=3072, L=512, B=8, vocab=30522)
MODES = ("hf_f32", "hf_bf16", "hip_f32", "hip_bf16")


def flops():
    s = SHAPE
    per_layer = 8 * s["L"] * s["d"] ** 2 + 4 * s["L"] ** 2 * s["d"] + 4 * s["L"] * s["d"] * s["inter"]
    return 3 * s["B"] * s["layers"] * per_layer


def one(mode, steps, warmup, repeats, embeddings="torch"):
    import torch
    from transformers import BertConfig, BertModel

    import bpmult_amd  # noqa: F401
    from bpmult_amd.models.bert import BertEmbeddingsHip, BertLayerStack, run_encoder, run_layers
    if not torch.cuda.is_available():
        raise SystemExit("text_encoder_step: needs a GPU (no CPU timing is meaningful)")
    s = SHAPE
    torch.manual_seed(1234)
    bert = BertModel(BertConfig(vocab_size=s["vocab"], hidden_size=s["d"], num_hidden_layers=s["layers"], num_attention_heads=s["heads"],
                                intermediate_size=s["inter"], max_position_embeddings=s["L"])).cuda().train()
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, s["vocab"], (s["B"], s["L"]), generator=g).cuda()
    mask, seg = torch.ones_like(ids), torch.zeros_like(ids)
    w = torch.randn(s["B"], s["L"], s["d"], generator=g).cuda()
    hip = mode.startswith("hip")
    stack = BertLayerStack(bert, "bf16" if mode == "hip_bf16" else "f32") if hip else None
    hip_emb = hip and embeddings == "hip"
    embd = BertEmbeddingsHip(bert, torch.zeros(1, device="cuda", dtype=torch.int32)) if hip_emb else None
    seed = [0]

    def step():
        for p in bert.parameters():
            p.grad = None
        if hip:
            seed[0] += 1
            stack.invalidate_shadows()          # a training step moves every weight: the bf16 / f32 shadows are re-packed per step
            if hip_emb:
                out = run_encoder(stack, embd, ids, mask, seg, seed[0], True)
            else:
                emb = bert.embeddings(input_ids=ids, token_type_ids=seg)
                out = run_layers(stack, emb, mask, seed[0], True)
        else:
            with torch.autocast("cuda", dtype=torch.bfloat16, enabled=mode == "hf_bf16"):
                out = bert(input_ids=ids, attention_mask=mask, token_type_ids=seg, return_dict=False)[0]
        (out.float() * w).sum().backward()

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    windows = []
    for _ in range(repeats):
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / steps)
    windows.sort()
    med = windows[len(windows) // 2]
    if hip_emb:
        assert int(embd.bad) == 0
        mode += "_hip_embeddings"
    print(json.dumps({"mode": mode, "ms_per_step": round(med, 3), "windows_ms": [round(x, 3) for x in windows],
                      "spread": round((windows[-1] - windows[0]) / med, 4), "tflops": round(flops() / (med * 1e-3) / 1e12, 1)}), flush=True)


def one_optimizer(text_params, steps, warmup, repeats):
    """forward + backward + FusedAdam.step() with the text parameters on the torch tail optimizer or in the flat store"""
    from types import SimpleNamespace

    import torch
    from transformers import BertConfig, BertModel

    import bpmult_amd  # noqa: F401
    from bpmult_amd.models import get_model
    from bpmult_amd.optim import FusedAdam
    if not torch.cuda.is_available():
        raise SystemExit("text_encoder_step: needs a GPU (no CPU timing is meaningful)")
    s = SHAPE
    torch.manual_seed(1234)
    a = SimpleNamespace(model="mmtrvat", orig_d_l=s["d"], orig_d_v=35, orig_d_a=74, orig_d_p=64, hidden_sz=24, vonly=True, lonly=True,
                        aonly=True, num_heads=4, layers=1, attn_dropout=0., attn_dropout_v=0., attn_dropout_a=0., relu_dropout=0.,
                        res_dropout=0., out_dropout=0., embed_dropout=0., attn_mask=True, hybrid=False, n_classes=6, bert_model="unused",
                        text_features=True, num_vectors_l=s["L"], num_vectors_a=48, num_vectors_v=48, precision="bf16",
                        text_encoder="hip", text_embeddings="hip", text_params=text_params)
    model = get_model(a)
    # a randomly initialised bert-base in place of BertModel.from_pretrained(directory): nothing is read or downloaded
    model.enc.bert = BertModel(BertConfig(vocab_size=s["vocab"], hidden_size=s["d"], num_hidden_layers=s["layers"],
                                          num_attention_heads=s["heads"], intermediate_size=s["inter"], max_position_embeddings=s["L"]))
    model.enc.features_in = False
    model = model.cuda().train()
    g = torch.Generator().manual_seed(5)
    ids = torch.randint(1, s["vocab"], (s["B"], s["L"]), generator=g).cuda()
    mask, seg = torch.ones_like(ids), torch.zeros_like(ids)
    img, aud = torch.randn(s["B"], 40, 35, generator=g).cuda(), torch.randn(s["B"], 31, 74, generator=g).cuda()
    tgt = (torch.randn(s["B"], 6, generator=g) > 0).float().cuda()
    opt = FusedAdam(model, lr=1e-4, fused_zero_grad=True)

    def fwd_bwd():
        torch.nn.functional.binary_cross_entropy_with_logits(model(ids, mask, seg, img, aud), tgt).backward()

    def step():
        fwd_bwd()
        opt.step()
        if opt._tail_opt is not None:                # (the flat buffers are cleared by the fused step)
            opt._tail_opt.zero_grad(set_to_none=False)

    for _ in range(warmup):
        step()
    torch.cuda.synchronize()
    windows, alloc = [], []
    for _ in range(repeats):
        b0 = torch.cuda.memory_stats()["allocated_bytes.all.allocated"]
        e0, e1 = torch.cuda.Event(enable_timing=True), torch.cuda.Event(enable_timing=True)
        e0.record()
        for _ in range(steps):
            step()
        e1.record()
        torch.cuda.synchronize()
        windows.append(e0.elapsed_time(e1) / steps)
        alloc.append((torch.cuda.memory_stats()["allocated_bytes.all.allocated"] - b0) // steps)
    windows.sort()
    med = windows[len(windows) // 2]
    stores = model._flat_stores()
    tail = [p for tg in opt._tail_opt.param_groups for p in tg["params"]] if opt._tail_opt is not None else []
    res = {"mode": text_params, "ms_per_step": round(med, 3), "windows_ms": [round(x, 3) for x in windows],
           "spread": round((windows[-1] - windows[0]) / med, 4), "allocated_bytes_per_step": sorted(alloc)[len(alloc) // 2],
           "flat_stores": len(stores), "flat_elements": [st.total for st in stores], "tail_tensors": len(tail),
           "tail_elements": sum(p.numel() for p in tail), "bad_token_ids": int(model.enc.bad_token_ids)}
    fwd_bwd()
    torch.cuda.synchronize()
    try:                                             # device kernels of one optimizer step
        from torch.profiler import ProfilerActivity, profile
        with profile(activities=[ProfilerActivity.CUDA]) as prof:
            opt.step()
            torch.cuda.synchronize()
        res["optimizer_step_kernels"] = sum(1 for e in prof.events() if "cuda" in str(e.device_type).lower())
    except Exception as e:                           # noqa: BLE001 -- the timing above stands without the count
        res["optimizer_step_kernels"] = None
        res["optimizer_step_kernels_error"] = f"{type(e).__name__}: {e}"[:200]
    print(json.dumps(res), flush=True)


def main_optimizer(a):
    res = dict(SHAPE, steps=a.steps, warmup=a.warmup, repeats=a.repeats, dropout=0.1, precision="bf16", text_embeddings="hip",
               trunk="mmtrvat hidden 24, 1 layer", step="forward + backward + FusedAdam.step(fused_zero_grad)", runs=[])
    for mode in ("torch", "flat") * a.rounds:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one-optimizer", mode, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats)]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:              # a time limit, a fault, an abort: nothing more is started on the device
            print(f"text_encoder_step: text_params {mode} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        res["runs"].append(json.loads([ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]))
    med = lambda mode: sorted(x["ms_per_step"] for x in res["runs"] if x["mode"] == mode)[(a.rounds - 1) // 2]
    res["ms_per_step"] = {"torch": med("torch"), "flat": med("flat")}
    res["torch_over_flat"] = round(med("torch") / med("flat"), 3)      # > 1: the flat store is faster
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--steps", type=int, default=40)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--repeats", type=int, default=3)
    ap.add_argument("--timeout", type=int, default=240, help="seconds per mode (child process)")
    ap.add_argument("--out", default=None, help="also write the result as JSON here")
    ap.add_argument("--embeddings", default="torch", choices=("torch", "hip"), help="embeddings of the hip_* modes")
    ap.add_argument("--modes", default=",".join(MODES), help="comma-separated subset of " + ",".join(MODES))
    ap.add_argument("--one", default=None, choices=MODES, help=argparse.SUPPRESS)
    ap.add_argument("--optimizer", action="store_true", help="the whole step with FusedAdam: text_params torch against flat")
    ap.add_argument("--rounds", type=int, default=2, help="--optimizer: how often the two settings alternate")
    ap.add_argument("--one-optimizer", default=None, choices=("torch", "flat"), help=argparse.SUPPRESS)
    a = ap.parse_args()
    if a.one:
        return one(a.one, a.steps, a.warmup, a.repeats, a.embeddings)
    if a.one_optimizer:
        return one_optimizer(a.one_optimizer, a.steps, a.warmup, a.repeats)
    if a.optimizer:
        return main_optimizer(a)
    modes = [m for m in a.modes.split(",") if m]
    if any(m not in MODES for m in modes):
        ap.error(f"--modes: a subset of {MODES}")
    res = dict(SHAPE, steps=a.steps, warmup=a.warmup, repeats=a.repeats, dropout=0.1, gflop_per_step=round(flops() / 1e9, 1), modes={})
    if a.out and os.path.exists(a.out):    # modes that are not run now keep their recorded figures
        res["modes"] = json.load(open(a.out)).get("modes", {})
    for mode in modes:
        cmd = ["timeout", "-k", "10", str(a.timeout), sys.executable, os.path.abspath(__file__), "--one", mode, "--steps", str(a.steps),
               "--warmup", str(a.warmup), "--repeats", str(a.repeats), "--embeddings", a.embeddings]
        r = subprocess.run(cmd, stdout=subprocess.PIPE, text=True)
        if r.returncode != 0:              # a time limit, a fault, an abort: nothing more is started on the device
            print(f"text_encoder_step: mode {mode} ended with status {r.returncode}; stopping", file=sys.stderr)
            return r.returncode
        line = [ln for ln in r.stdout.splitlines() if ln.startswith("{")][-1]
        m = json.loads(line)
        res["modes"][m.pop("mode")] = m
    md = res["modes"]
    ratio = lambda a_, b_: round(md[a_]["ms_per_step"] / md[b_]["ms_per_step"], 3) if a_ in md and b_ in md else None
    res["hip_bf16_over_hf_bf16"] = ratio("hf_bf16", "hip_bf16")      # > 1: the HIP path is faster
    res["hip_f32_over_hf_f32"] = ratio("hf_f32", "hip_f32")
    res["hip_embeddings_over_torch_embeddings_bf16"] = ratio("hip_bf16", "hip_bf16_hip_embeddings")   # > 1: HIP embeddings are faster
    print(json.dumps(res))
    if a.out:
        with open(a.out, "w") as f:
            json.dump(res, f, indent=1)
            f.write("\n")
    return 0


if __name__ == "__main__":
    sys.exit(main())
