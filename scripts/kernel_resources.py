#!/usr/bin/env python3
"""Per-kernel resource table of the HIP sources: compiles each .hip file device-only to assembly with the Makefile's
flags and prints, for every kernel, the registers, scratch and LDS the code object's metadata records.

    python scripts/kernel_resources.py [--src DIR] [--out FILE] [file.hip ...]      # one table
    python scripts/kernel_resources.py --diff OLD.txt NEW.txt                      # the kernels whose values differ

Needs hipcc only (no GPU).  Columns: file  kernel  vgpr  sgpr  scratch bytes  LDS bytes.
"""
import argparse
import concurrent.futures
import os
import re
import subprocess
import sys
import tempfile

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "--cuda-device-only", "-S"]
FIELDS = [".vgpr_count", ".sgpr_count", ".private_segment_fixed_size", ".group_segment_fixed_size"]


def kernels_of(path):
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    with tempfile.TemporaryDirectory() as tmp:
        out = os.path.join(tmp, "a.s")
        subprocess.check_call([hipcc] + FLAGS + [path, "-o", out], stderr=subprocess.DEVNULL)
        text = open(out).read()
    meta = text[text.index("amdhsa.kernels:"):]
    rows = []
    # one metadata record per kernel: the keys of a record are sorted, a record ends where the next list item begins
    for rec in re.split(r"\n  - \.agpr_count:", meta)[1:]:
        vals = {k: re.search(r"\n    %s:\s*(\S+)" % re.escape(k), rec).group(1) for k in FIELDS + [".name"]}
        if vals[".name"].startswith("_ZN4ipxk"):      # the project's kernels (not the sort / scan kernels a library instantiates)
            rows.append((os.path.basename(path), vals[".name"]) + tuple(int(vals[k]) for k in FIELDS))
    return rows


def table(src, files, jobs):
    if not files:
        files = sorted(f for f in os.listdir(src) if f.endswith(".hip"))
    paths = [os.path.join(src, f) for f in files]
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        rows = [r for rs in pool.map(kernels_of, paths) for r in rs]
    return ["%s %s %d %d %d %d" % r for r in sorted(rows)]


def diff(old, new):
    def load(p):
        return {tuple(l.split()[:2]): l.split()[2:] for l in open(p) if l.strip() and not l.startswith("#")}
    a, b = load(old), load(new)
    print("# file kernel: vgpr sgpr scratch lds, %s -> %s" % (os.path.basename(old), os.path.basename(new)))
    changed = 0
    for k in sorted(set(a) | set(b)):
        if a.get(k) != b.get(k):
            changed += 1
            print("%s %s: %s -> %s" % (k[0], k[1], " ".join(a.get(k, ["absent"])), " ".join(b.get(k, ["absent"]))))
    print("# %d kernels in %s, %d in %s, %d differ" % (len(a), os.path.basename(old), len(b), os.path.basename(new), changed))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--src", default=os.path.join(ROOT, "ipx_amd", "csrc"))
    ap.add_argument("--out")
    ap.add_argument("--jobs", type=int, default=4)
    ap.add_argument("--diff", nargs=2, metavar=("OLD", "NEW"))
    ap.add_argument("files", nargs="*")
    args = ap.parse_args()
    if args.diff:
        return diff(*args.diff)
    lines = ["# file kernel vgpr sgpr scratch_bytes lds_bytes   (hipcc %s)" % " ".join(FLAGS)] + table(args.src, args.files, args.jobs)
    if args.out:
        with open(args.out, "w") as f:
            f.write("\n".join(lines) + "\n")
    else:
        print("\n".join(lines))


if __name__ == "__main__":
    sys.exit(main())
