#!/usr/bin/env python3
"""Generate the head_dim > 128 fixtures F13 / F14 from the REAL reference, with the harness of make_golden.py (its shims,
deterministic weights / inputs and fixture layout; that file is imported, not changed).

  F13: mmtrvat  d=512, 2 heads (head_dim 256), 2 layers, B=2, L/V/A = 20/60/50 -> num_vectors 64 (zero-padded lengths)
  F14: mmtrvapt d=384, 2 heads (head_dim 192: zero padding to 256), 2 layers, B=2, the shapes of F8

usage:  python tests/golden/make_golden_wide_heads.py [--only f13,f14]
"""
import argparse
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, HERE)
import make_golden as mg  # noqa: E402  (applies the reference shims)


def f13_wide_mmtrvat():
    mg._three_modal("f13_wide_mmtrvat", "f13.", 512, 2, 2, 2, 20, 60, 50, 32, small_only=True, nv=64)


def f14_wide_mmtrvapt():
    pfx = "f14."
    d, H, Ly, B = 384, 2, 2, 2
    mg.torch.manual_seed(0)
    args = mg._args(hidden_sz=d, num_heads=H, layers=Ly, orig_d_l=32, orig_d_v=40, orig_d_a=96, orig_d_p=64, n_classes=13)
    model = mg.mmtr.MultiprojectionMMTransformerGMUClf(args)
    model.train()
    xl, img = mg.leaf(pfx + "xl", (B, 60, 32)), mg.leaf(pfx + "img", (B, 150, 40))
    aud, post = mg.leaf(pfx + "aud", (B, 96, 1000)), mg.leaf(pfx + "post", (B, 64))
    model.enc.feat = xl
    call = lambda: model(None, None, None, img, aud, post, output_gate=True)
    full = ["out_layer.weight", "out_layer.bias", "proj2.bias", "gmu.x4_gate.weight", "transfm_l2v.bias",
            "trans_l_with_a.layers.0.self_attn.in_proj_bias", "trans_a_with_v.layers.0.fc2.bias",
            "trans_v_with_l2a.layers.0.layer_norms.0.weight", "trans_a_with_l2v.layers.1.layer_norms.1.bias",
            "trans_l_with_v2a.layers.1.layer_norms.2.weight", "trans_a_with_v2l.layer_norm.weight",
            "trans_v_with_l.layers.0.self_attn.out_proj.bias", "trans_v_with_a2l.layers.1.self_attn.in_proj_bias"]
    mg._model_fixture("f14_wide_mmtrvapt", model, pfx, call, {"xl": xl, "img": img, "post": post}, 13, full, small_only=True)


ALL = dict(f13=f13_wide_mmtrvat, f14=f14_wide_mmtrvapt)

if __name__ == "__main__":
    ap = argparse.ArgumentParser()
    ap.add_argument("--only", default="")
    a = ap.parse_args()
    mg.torch.set_num_threads(8)
    for k, fn in ALL.items():
        if a.only and k not in a.only.split(","):
            continue
        print(k)
        fn()
