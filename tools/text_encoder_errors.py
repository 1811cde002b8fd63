"""Measure what HF BertModel itself achieves on the device against its own fp64 CPU values, on the inputs of
tests/test_text_encoder_gpu.py, and write profiles/text_encoder_errors.json -- the figures that test multiplies into its
tolerances (4 x HF fp32 for the f32 mode, 2 x HF under bf16 autocast for the bf16 mode).  The HIP path's own errors are
recorded next to them for information; no tolerance is derived from them.

    python tools/text_encoder_errors.py            # on an MI355X, after build()
"""
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
import test_text_encoder_gpu as T  # noqa: E402


def strip(e):
    r = lambda v: float(f"{v:.4e}")
    return {k: (r(v) if isinstance(v, float) else {n: r(x) for n, x in v.items()} if isinstance(v, dict) else v) for k, v in e.items()}


def main():
    out = {"_about": "max|got-ref| / max(max|ref|, floor) per tensor class against HF fp64 on the CPU; see tests/test_text_encoder_gpu.py",
           "device": torch.cuda.get_device_name(0), "torch": torch.__version__}
    for case in T.CASES:
        bert, dev_in, ref = T.reference(case)
        out[case] = {
            "hf_f32": strip(T.errors(T.run_hf(bert, *dev_in), ref)),
            "hf_bf16": strip(T.errors(T.run_hf(bert, *dev_in, autocast=True), ref)),
            "hip_f32": strip(T.errors(T.run_hip(bert, *dev_in, "f32"), ref)),
            "hip_bf16": strip(T.errors(T.run_hip(bert, *dev_in, "bf16"), ref)),
        }
        print(case, json.dumps({k: T.brief(v) for k, v in out[case].items()}), flush=True)
        for prec, hf in (("f32", "hf_f32"), ("bf16", "hf_bf16")):          # information: where the HIP path stands, per parameter
            ratio = {n: out[case]["hip_" + prec]["per"][n] / max(out[case][hf]["per"][n], 1e-300) for n in out[case][hf]["per"]}
            w = max(ratio, key=ratio.get)
            print(f"  {case}/{prec}: largest hip / hf ratio of a parameter gradient {ratio[w]:.2f} ({w})", flush=True)
    # model level: the torch text encoder in fp32 against the same model with BERT in fp64 (features cast to fp32 in front
    # of the trunk), and the torch path against itself
    with tempfile.TemporaryDirectory() as tmp:
        m_h, m_t = T.build_models(pathlib.Path(tmp))
        m_h.use_graphs = m_t.use_graphs = False
        x = T.model_inputs()
        r32 = T.model_step(m_t, x)
        again = T.model_step(m_t, x)
        hip = T.model_step(m_h, x)
        m_t.enc.bert.double()
        r64 = T.model_step(m_t, x)
        out["model"] = {"hf_f32_vs_f64_text": strip(T.model_errors(r32, r64)), "torch_run_to_run": strip(T.model_errors(again, r32)),
                        "hip_vs_torch": strip(T.model_errors(hip, r32))}
        print("model", json.dumps({k: T.brief(v) for k, v in out["model"].items()}), flush=True)
        a, b, h = (out["model"][k]["per"] for k in ("hf_f32_vs_f64_text", "torch_run_to_run", "hip_vs_torch"))
        ratio = {n: h[n] / max(a[n], b[n], 1e-300) for n in h}
        w = max(ratio, key=ratio.get)
        print(f"  model: largest hip-vs-torch / recorded ratio of a parameter gradient {ratio[w]:.2f} ({w})", flush=True)
    path = os.path.join(ROOT, "profiles", "text_encoder_errors.json")
    with open(path, "w") as f:
        json.dump(out, f, indent=1)
        f.write("\n")
    print("wrote", path)


if __name__ == "__main__":
    main()
