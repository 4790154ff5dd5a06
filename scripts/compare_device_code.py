#!/usr/bin/env python3
"""Compare the gfx950 device code of two source trees, kernel by kernel.

    scripts/compare_device_code.py OLD_TREE NEW_TREE [--jobs N] [--keep DIR]

Every csrc/hip/*.hip of both trees is compiled with the library's flags plus `--cuda-device-only -S`.  The assembly is
split at kernel symbols; per kernel the instruction text (comments dropped, the per-file function number in local labels
normalised) and the .amdhsa_ resource block are compared.  Reported: kernels only one tree has, kernels that now come
out of more translation units than before, kernels whose text or resources differ.  Exit status 0 only when none.
No GPU is needed.
"""
import argparse
import concurrent.futures
import glob
import os
import re
import subprocess
import sys
import tempfile

FLAGS = ["--offload-arch=gfx950", "-O3", "-std=c++17", "-ffp-contract=off", "-Wall", "-Wno-unused-function",
         "--cuda-device-only", "-S"]
LOCAL = re.compile(r"\.L(BB|func_end|func_begin|tmp|JTI)\d+")


def compile_tu(tree, src, out):
    subprocess.check_call([os.environ.get("HIPCC", "hipcc"), *FLAGS, "-I" + os.path.join(tree, "include"), "-o", out, src])
    return out


def kernels_of(asm_path):
    """{kernel: (instruction text, resource block)} of one assembly file"""
    lines = open(asm_path).read().split("\n")
    names, res = [], {}
    i = 0
    while i < len(lines):
        m = re.match(r"\s*\.amdhsa_kernel\s+(\S+)", lines[i])
        if m:
            j = i
            while not lines[j].strip().startswith(".end_amdhsa_kernel"):
                j += 1
            names.append(m.group(1))
            res[m.group(1)] = "\n".join(l.strip() for l in lines[i + 1:j])
            i = j
        i += 1
    out = {}
    for name in names:
        start = next(i for i, l in enumerate(lines) if l.startswith(name + ":"))
        body = []
        for l in lines[start + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].rstrip()
            if l.strip():
                body.append(LOCAL.sub(lambda m: ".L" + m.group(1), l))
        out[name] = ("\n".join(body), res[name])
    return out


def tree_kernels(tree, tmp, tag, jobs):
    srcs = sorted(glob.glob(os.path.join(tree, "spmv_openmp_cuda_amd", "csrc", "hip", "*.hip")))
    with concurrent.futures.ThreadPoolExecutor(jobs) as pool:
        outs = list(pool.map(lambda s: compile_tu(tree, s, os.path.join(tmp, tag + "_" + os.path.basename(s) + ".s")), srcs))
    table = {}                                       # kernel -> [(file, text, resources)]
    for src, out in zip(srcs, outs):
        for k, (text, res) in kernels_of(out).items():
            table.setdefault(k, []).append((os.path.basename(src), text, res))
    return table


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--jobs", type=int, default=8)
    ap.add_argument("--keep", help="keep the assembly files in this directory")
    a = ap.parse_args()
    tmp = a.keep or tempfile.mkdtemp(prefix="devcode_")
    os.makedirs(tmp, exist_ok=True)
    old, new = tree_kernels(a.old, tmp, "old", a.jobs), tree_kernels(a.new, tmp, "new", a.jobs)
    bad = 0
    for k in sorted(set(old) | set(new)):
        if k not in new or k not in old:
            print("ONLY IN %s: %s" % ("OLD" if k in old else "NEW", k)); bad += 1
            continue
        if len(new[k]) > len(old[k]):
            print("MORE COPIES: %s: %s -> %s" % (k, [f for f, _, _ in old[k]], [f for f, _, _ in new[k]])); bad += 1
        # a kernel's copies may differ from file to file within one tree (a library template under another file's macros):
        # every copy of the new tree must be the text of some copy of the old one, and likewise its resources
        for f, text, res in new[k]:
            if text not in [t for _, t, _ in old[k]]:
                print("TEXT DIFFERS: %s (%s)" % (k, f)); bad += 1
            if res not in [r for _, _, r in old[k]]:
                print("RESOURCES DIFFER: %s (%s)" % (k, f)); bad += 1
    print("%d kernels in the old tree, %d in the new; %d kernel copies old, %d new; %d differences" %
          (len(old), len(new), sum(map(len, old.values())), sum(map(len, new.values())), bad))
    return 1 if bad else 0


if __name__ == "__main__":
    sys.exit(main())
