#!/usr/bin/env python
"""Which `s_waitcnt vmcnt` instructions sit in the k loop of each gemm_dma_kernel instantiation?  Needs hipcc, no GPU.

    python tools/gemm_dma_loop_waits.py [--tree DIR] [--parent DIR] [--out profiles/gemm_dma_loop_waits.json]

csrc/gemm.hip of each tree is compiled device-only to assembly (the flags of _lib.build, as tools/kernel_isa_diff.py
does).  In every gemm_dma_kernel symbol the k loop is the union of the loops (label ... backward branch) that hold an
MFMA; each `s_waitcnt` with a vmcnt field inside it is listed with its loop-relative instruction index and classed as
  hand      inside an ;;#ASMSTART ... ;;#ASMEND block (dma_wait<N> of csrc/gemm_dma.h)
  compiler  anywhere else: inserted by the compiler's wait-count pass.  Between the request of an LDS-DMA stage and its
            counted wait such a wait drains the stage ring.
The record also counts the loop's MFMAs, LDS-DMA requests and transposed LDS reads so that a reader can see which
loop was measured.  Exit status 0 when the tree (--tree) has no compiler-inserted wait in any k loop."""
import argparse
import json
import os
import re
import subprocess
import sys
import tempfile

PKG = "biprojection-multimodal-transformer_amd"
ARCH = "gfx950"                      # == _lib.ARCH
FLAGS = ["-O3", "-std=c++17", "-fPIC"]
ARGS = ("XK", "YK", "WMD", "WND", "TMW", "NS", "XS", "X3", "DKT")


def compile_asm(root, tmp, tag):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    out = os.path.join(tmp, f"{tag}_gemm.s")
    subprocess.run([hipcc, f"--offload-arch={ARCH}", *FLAGS, "--cuda-device-only", "-S",
                    os.path.join(root, PKG, "csrc", "gemm.hip"), "-o", out], check=True, stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def instantiation(sym):
    m = re.search(r"gemm_dma_kernelI((?:L[bi]\d+E)+)E", sym)
    vals = [int(v) for v in re.findall(r"L[bi](\d+)E", m.group(1))]
    a = dict(zip(ARGS, vals))
    form = "NT" if a["XK"] and a["YK"] else "NN" if a["XK"] else "TN"
    name = f"{form} {16 * a['TMW'] * a['WMD']}x{64 * a['WND']} waves {a['WMD']}x{a['WND']} NS{a['NS']} DKT{a['DKT']}"
    return name + (" XS" if a["XS"] else "") + (" X3" if a["X3"] else ""), a


def kernel_lines(asm):
    """symbol -> its instruction / label / asm-marker lines"""
    lines = asm.split("\n")
    out = {}
    for sym in re.findall(r"^\s*\.amdhsa_kernel\s+(\S*gemm_dma_kernel\S*)", asm, flags=re.M):
        start = next(i for i, ln in enumerate(lines) if ln.startswith(sym + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".Lfunc_end"))
        out[sym] = lines[start + 1:end]
    return out


def loop_waits(body):
    code = []                                       # (text, inside an asm block)
    in_asm = False
    for ln in body:
        s = ln.strip()
        if s.startswith(";;#ASMSTART"):
            in_asm = True
        elif s.startswith(";;#ASMEND"):
            in_asm = False
        s = re.split(r"\s*(?:;|//)", s, 1)[0].strip()
        if s and (not s.startswith(".") or re.match(r"\.L\S+:", s)):
            code.append((re.sub(r"\s+", " ", s), in_asm))
    label_at = {m.group(1): i for i, (s, _) in enumerate(code) for m in [re.match(r"(\.L\S+):", s)] if m}
    lo, hi = None, None
    for i, (s, _) in enumerate(code):
        m = re.match(r"s_c?branch\S* (\.L\S+)", s)
        if not m or label_at.get(m.group(1), i + 1) > i:
            continue
        a = label_at[m.group(1)]
        if any(t.startswith("v_mfma") for t, _ in code[a:i]):
            lo, hi = a if lo is None else min(lo, a), i if hi is None else max(hi, i)
    if lo is None:
        return None
    loop = [c for c in code[lo:hi + 1] if not c[0].endswith(":")]
    rec = {"instructions": len(loop), "mfma": sum(s.startswith("v_mfma") for s, _ in loop),
           "lds_dma": sum(s.startswith("buffer_load") and s.endswith(" lds") for s, _ in loop),
           "ds_read_tr": sum(s.startswith("ds_read_b64_tr") for s, _ in loop), "hand": [], "compiler": []}
    for i, (s, asm) in enumerate(loop):
        if s.startswith("s_waitcnt") and "vmcnt" in s:
            rec["hand" if asm else "compiler"].append({"at": i, "text": s})
    return rec


def tree_record(root, tmp, tag):
    out = {}
    for sym, body in kernel_lines(compile_asm(root, tmp, tag)).items():
        name, args = instantiation(sym)
        out[name] = {"template": args, **loop_waits(body)}
    return dict(sorted(out.items()))


def main():
    here = os.path.join(os.path.dirname(os.path.abspath(__file__)), "..")
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--tree", default=here)
    ap.add_argument("--parent", help="a checkout of the parent commit, recorded beside the tree")
    ap.add_argument("--out")
    args = ap.parse_args()
    report = {"tool": "tools/gemm_dma_loop_waits.py", "arch": ARCH, "flags": FLAGS}
    with tempfile.TemporaryDirectory() as tmp:
        for key, root in (("parent", args.parent), ("tree", args.tree)):
            if root:
                ks = tree_record(root, tmp, key)
                report[key] = {"instantiations": len(ks), "compiler_waits_total": sum(len(k["compiler"]) for k in ks.values()),
                               "with_compiler_waits": [n for n, k in ks.items() if k["compiler"]], "kernels": ks}
    if args.out:
        with open(args.out, "w") as f:
            json.dump(report, f, indent=1)
            f.write("\n")
    for key in ("parent", "tree"):
        if key in report:
            r = report[key]
            print(f"{key}: {r['instantiations']} instantiations, {r['compiler_waits_total']} compiler-inserted vmcnt waits in k loops")
            for n in r["with_compiler_waits"]:
                print(f"  {n}: " + ", ".join(f"{w['text']} @{w['at']}" for w in r["kernels"][n]["compiler"]))
    sys.exit(0 if report["tree"]["compiler_waits_total"] == 0 else 1)


if __name__ == "__main__":
    main()
