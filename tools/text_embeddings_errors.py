"""Measure what HF's own fp32 `BertEmbeddings` achieve on the device against their fp64 CPU values, on the inputs of
tests/test_text_embeddings_gpu.py, and write profiles/text_embeddings_errors.json -- the figures that test multiplies by 4
into its tolerances (embedding output, dword, dpos, dtype, dgamma, dbeta; each tensor its own).  The HIP path's own errors
are recorded next to them for information; no tolerance is derived from them.

"small_encoder": the gradients of the embedding parameters THROUGH the HF layers ("small" case of
tests/test_text_encoder_gpu.py, HF BertModel fp32 on the device against fp64) -- the bound of the module-level test.

    python tools/text_embeddings_errors.py            # on an MI355X, after build()
"""
import copy
import json
import os
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
for p in (ROOT, os.path.join(ROOT, "tests")):
    if p not in sys.path:
        sys.path.insert(0, p)

import pathlib  # noqa: E402

import torch  # noqa: E402

import bpmult_amd  # noqa: E402,F401
import test_text_embeddings_gpu as E  # noqa: E402
import test_text_encoder_gpu as T  # noqa: E402


def r4(e):
    return {k: float(f"{v:.4e}") for k, v in e.items()}


def emb_grads(bert):
    return {n: p.grad.detach().double().cpu() for n, p in bert.named_parameters() if n.startswith("embeddings.")}


def main():
    out = {"_about": "max|got-ref| / max(max|ref|, floor) per tensor against HF fp64 on the CPU; see tests/test_text_embeddings_gpu.py",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    for case, seg_kind, pad, ids_kind in E.RECORDED:
        emb, cfg, (ids, seg, w), ref = E.reference(case, seg_kind, pad, ids_kind)
        c = E.CASES[case]
        key = E.key_of(case, seg_kind, pad, ids_kind)
        out[key] = {"hf_f32": r4(E.errors(E.run_hf_embeddings(emb, ids, seg, w), ref))}
        for prec in ("f32", "bf16"):
            out[key]["hip_" + prec] = r4(E.errors(E.HipEmbeddings(emb, cfg, c["B"], c["L"], prec).run(ids, seg, w), ref))
        print(key, json.dumps(out[key]), flush=True)
    # through the layers: HF BertModel fp32 on the device against fp64, embedding parameters only
    bert, (ids, mask, seg, w), _ = T.reference("small")
    b64 = copy.deepcopy(bert).cpu().double()
    T.run_hf(b64, ids.cpu(), mask.cpu(), seg.cpu(), w.cpu().double())
    ref = emb_grads(b64)
    T.run_hf(bert, ids, mask, seg, w)
    got = emb_grads(bert)
    floor = 1e-3 * max(float(p.grad.abs().max()) for n, p in b64.named_parameters() if p.grad is not None)
    rel = lambda a, b: float(f"{float((a - b).abs().max() / max(float(b.abs().max()), floor)):.4e}")
    out["small_encoder"] = {"hf_f32": {n: rel(got[n], ref[n]) for n in ref}}
    with tempfile.TemporaryDirectory() as tmp:             # information: the HIP encoder with HIP embeddings on the same inputs
        _, enc = E._encoders(pathlib.Path(tmp))
        _, g = E._enc_step(enc, ids, mask, seg, w)
        out["small_encoder"]["hip_f32"] = {n: rel(g[n], ref[n]) for n in ref}
    print("small_encoder", json.dumps(out["small_encoder"]), flush=True)
    path = os.path.join(ROOT, "profiles", "text_embeddings_errors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
