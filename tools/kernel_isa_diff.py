#!/usr/bin/env python
"""Do two trees compile to the same kernels?  Needs hipcc, no GPU.

    python tools/kernel_isa_diff.py A_DIR B_DIR [--out report.json] [--jobs 4] [--by-instantiation]

Every csrc/*.hip of both trees is compiled device-only to assembly (--cuda-device-only -S, otherwise the flags of
_lib.build) and each file is split at its kernel symbols.  For every kernel of either tree the report says whether
  code        the instruction text (comments dropped, local labels renumbered in order of appearance) and
  descriptor  its .amdhsa_kernel ... .end_amdhsa_kernel block (registers, LDS, scratch, ...)
are identical in the two builds, and which kernels only one tree has.  Kernels are matched by symbol over the whole
tree, so one that moved to another file still meets its counterpart.  Exit status 0 when the two sets of symbols are
equal and every kernel is identical in both respects.  It compares two builds; it looks for nothing inside them.
--by-instantiation matches kernels by name and template arguments alone (the mangled symbol without its parameter
types): a kernel whose argument TYPE was renamed or respelled, which changes its symbol and nothing
else, still meets its counterpart; the symbol inside the text is replaced by a placeholder on both sides."""
import argparse
import hashlib
import json
import os
import re
import subprocess
import sys
import tempfile
from concurrent.futures import ThreadPoolExecutor

PKG = "biprojection-multimodal-transformer_amd"
ARCH = "gfx950"                      # == _lib.ARCH
FLAGS = ["-O3", "-std=c++17", "-fPIC"]


def compile_asm(src, out):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc, f"--offload-arch={ARCH}", *FLAGS, "--cuda-device-only", "-S", src, "-o", out], check=True,
                   stderr=subprocess.DEVNULL)
    with open(out) as f:
        return f.read()


def strip_comment(line):
    return re.split(r"\s*(?:;|//)", line, 1)[0].rstrip()


def kernels_of(asm):
    """symbol -> (code text, descriptor text) of one assembly file"""
    names = re.findall(r"^\s*\.amdhsa_kernel\s+(\S+)", asm, flags=re.M)
    lines = asm.split("\n")
    out = {}
    for name in names:
        start = next(i for i, ln in enumerate(lines) if ln.startswith(name + ":"))
        end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith(".end_amdhsa_kernel"))
        body, desc, in_desc, in_code = [], [], False, True
        for ln in lines[start:end + 1]:
            s = strip_comment(ln).strip()
            if not s:
                continue
            if s.startswith(".amdhsa_kernel"):
                in_desc, in_code = True, False
            if in_desc:
                desc.append(re.sub(r"\s+", " ", s))
            elif in_code:
                if s.startswith("s_endpgm") or not s.startswith("."):
                    body.append(re.sub(r"\s+", " ", s))
                elif re.match(r"\.L\S+:", s):
                    body.append(s)
                if s.startswith(".Lfunc_end"):
                    in_code = False
        labels = {}
        for ln in body:                                   # local labels, numbered in order of definition
            m = re.match(r"(\.L[\w$.]+):", ln)
            if m and not m.group(1).startswith(".Lfunc_end"):
                labels.setdefault(m.group(1), f".L{len(labels)}")
        body = [ln for ln in body if not ln.startswith(".Lfunc_end")]
        text = "\n".join(re.sub(r"\.L[\w$.]+", lambda m: labels.get(m.group(0), m.group(0)), ln) for ln in body)
        out[name] = (text, "\n".join(desc))
    return out


def tree_kernels(root, jobs, tmp):
    csrc = os.path.join(root, PKG, "csrc")
    files = sorted(f for f in os.listdir(csrc) if f.endswith(".hip"))
    tag = hashlib.sha1(os.path.abspath(root).encode()).hexdigest()[:8]
    with ThreadPoolExecutor(max_workers=jobs) as ex:
        asms = list(ex.map(lambda f: compile_asm(os.path.join(csrc, f), os.path.join(tmp, f"{tag}_{f[:-4]}.s")), files))
    seen = {}
    for f, asm in zip(files, asms):
        for name, (code, desc) in kernels_of(asm).items():
            seen.setdefault(name, []).append({"file": f, "code": code, "desc": desc})
    # a kernel of a shared header (unnamed namespace) that several files instantiate has one symbol per file: those are
    # matched as symbol@file
    found = {}
    for name, ks in seen.items():
        for k in ks:
            found[name if len(ks) == 1 else f"{name}@{k['file']}"] = k
    return found


def by_instantiation(found):
    """found, keyed by the mangled name up to the end of the template arguments (the parameter types cut off)"""
    out = {}
    for sym, k in found.items():
        m = re.match(r"(_ZN.*?EE)v", sym) or re.match(r"(_Z\d+\w+?I.*?E)v", sym)       # nested (namespace) name / plain name
        key = m.group(1) if m else sym
        assert key not in out, key
        out[key] = {"file": k["file"], "code": k["code"].replace(sym, "<kernel>"), "desc": k["desc"].replace(sym, "<kernel>")}
    return out


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("a_dir")
    ap.add_argument("b_dir")
    ap.add_argument("--out", help="write the report (JSON) here")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--by-instantiation", action="store_true", help="match kernels by name and template arguments, not by symbol")
    args = ap.parse_args()
    with tempfile.TemporaryDirectory() as tmp:
        a, b = tree_kernels(args.a_dir, args.jobs, tmp), tree_kernels(args.b_dir, args.jobs, tmp)
    if args.by_instantiation:
        a, b = by_instantiation(a), by_instantiation(b)
    both = sorted(set(a) & set(b))
    kernels = {k: {"a_file": a[k]["file"], "b_file": b[k]["file"], "code_identical": a[k]["code"] == b[k]["code"],
                   "descriptor_identical": a[k]["desc"] == b[k]["desc"], "instructions": a[k]["code"].count("\n") + 1,
                   "code_sha256": hashlib.sha256(b[k]["code"].encode()).hexdigest()[:16]} for k in both}
    report = {
        "tool": "tools/kernel_isa_diff.py A_DIR B_DIR" + (" --by-instantiation" if args.by_instantiation else ""), "arch": ARCH, "flags": FLAGS,
        "kernels_a": len(a), "kernels_b": len(b), "only_in_a": sorted(set(a) - set(b)), "only_in_b": sorted(set(b) - set(a)),
        "identical": sum(v["code_identical"] and v["descriptor_identical"] for v in kernels.values()),
        "different": sorted(k for k, v in kernels.items() if not (v["code_identical"] and v["descriptor_identical"])),
        "kernels": kernels,
    }
    if args.out:
        with open(args.out, "w") as f:
            head = json.dumps({k: v for k, v in report.items() if k != "kernels"}, separators=(",", ":"))
            rows = ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in kernels.items())
            f.write(head[:-1] + ',"kernels":{\n' + rows + "\n}}\n")                 # a kernel per line
    print(json.dumps({k: v for k, v in report.items() if k != "kernels"}, indent=1))
    ok = not report["only_in_a"] and not report["only_in_b"] and not report["different"]
    sys.exit(0 if ok else 1)


if __name__ == "__main__":
    main()
