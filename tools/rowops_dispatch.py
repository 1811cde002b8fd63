#!/usr/bin/env python
"""Which kernel, grid and block every row-kernel / Adam entry point (--cases rowops: tests/rowops_cases.py) or attention
entry point (--cases attn: tests/attn_cases.py) launches, for each case of the table, asked of a -DBPM_LAB build in dry
mode (bpm_debug_rows_dry / bpm_debug_rows_last): needs no GPU, launches nothing.

    python tools/rowops_dispatch.py [--cases attn]                  # this tree's lab build, printed
    python tools/rowops_dispatch.py [--cases attn] --lib L.so --out F    # another tree's lab build, written to F

profiles/rowops_dispatch.json is the second form run on the tree that still had csrc/rowops.hip, given the two query
functions by profiles/rowops_parent_dispatch_hook.patch; profiles/attn_dispatch.json the same on the tree that still had
all of attention in csrc/attention.hip, whose launches profiles/attn_parent_dispatch_hook.patch routes to the query.
tests/test_rowops_dispatch_cpu.py and tests/test_attn_dispatch_cpu.py compare this tree with them."""
import argparse
import importlib
import json
import os
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path[:0] = [ROOT, os.path.join(ROOT, "tests")]

import bpmult_amd  # noqa: E402,F401
from bpmult_amd import _lib  # noqa: E402


def main():
    ap = argparse.ArgumentParser(description=__doc__.split("\n\n")[0])
    ap.add_argument("--cases", choices=("rowops", "attn"), default="rowops", help="the case table: tests/<cases>_cases.py")
    ap.add_argument("--lib", help="a -DBPM_LAB build of the library (default: build this tree's)")
    ap.add_argument("--out", help="write the record here instead of printing it")
    args = ap.parse_args()
    cases = importlib.import_module(args.cases + "_cases")
    L = _lib.bind_lab(_lib.load(args.lib or _lib.build_lab()))
    record = cases.run_all(L)
    text = "{\n" + ",\n".join(json.dumps(k) + ":" + json.dumps(v, separators=(",", ":")) for k, v in record.items()) + "\n}\n"      # a case per line
    if args.out:
        with open(args.out, "w") as f:
            f.write(text)
        print(f"{len(record)} cases, {sum(len(r['launches']) for r in record.values())} launches -> {args.out}")
    else:
        sys.stdout.write(text)


if __name__ == "__main__":
    main()
