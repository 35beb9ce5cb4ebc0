#!/usr/bin/env python3
"""Register, scratch, occupancy and LDS figures of every kernel of one csrc/*.hip file.

    python scripts/kernel_resources.py csrc/fa_decode.hip [csrc/fa_kvq.hip ...] [--match TEXT]

Compiles the device side of each file with the command the Makefile uses for its object (asked
of `make -n`, so HIPFLAGS and the file's EXTRA_FLAGS are the product's) plus
-Rpass-analysis=kernel-resource-usage, and prints one table row per kernel, sorted by name, in
the layout of profiles/decode_kernels_resources.txt. Needs hipcc, no GPU.
"""
import argparse
import os
import re
import shlex
import shutil
import subprocess
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PKG = os.path.join(ROOT, "llmsys-project-flashattn_amd")

FIELDS = (("VGPRs", "VGPR"), ("AGPRs", "AGPR"), ("TotalSGPRs", "SGPR"), ("ScratchSize [bytes/lane]", "scratch B/lane"),
          ("Occupancy [waves/SIMD]", "waves/SIMD"), ("LDS Size [bytes/block]", "LDS B/block"))


def compile_command(src, pkg):
    """The Makefile's hipcc line for build/<name>.o, as a list, without -c / -o."""
    name = os.path.splitext(os.path.basename(src))[0]
    out = subprocess.run(["make", "-n", "-B", f"build/{name}.o"], cwd=pkg, check=True, capture_output=True,
                         text=True).stdout
    line = next(ln for ln in out.splitlines() if f"csrc/{name}.hip" in ln and " -c " in ln)
    argv = shlex.split(line)
    drop = argv.index("-o")
    del argv[drop:drop + 2]
    argv.remove("-c")
    return argv


def short_name(mangled, filt):
    s = subprocess.run([filt, mangled], check=True, capture_output=True, text=True).stdout.strip()
    if s == mangled and "DF16b" in mangled:
        # a demangler older than the bf16 mangling: DF16b -> Dh ("half"), a builtin type like it, so
        # the substitution indices of the rest of the name hold
        s = subprocess.run([filt, mangled.replace("DF16b", "Dh")], check=True, capture_output=True, text=True).stdout
        s = s.strip().replace("half", "__bf16")
    s = re.sub(r"^void ", "", s)
    depth, cut = 0, len(s)
    for i, ch in enumerate(s):  # drop the parameter list: the first "(" outside template brackets
        depth += ch == "<"
        depth -= ch == ">"
        if ch == "(" and depth == 0:
            cut = i
            break
    s = s[:cut].replace("mt::", "").replace("__bf16", "bf16")
    return s.replace("<true>", "<fp8>").replace("<false>", "<bf16>") if s.startswith("kvq_append") else s


def resources(src, pkg):
    argv = compile_command(src, pkg) + ["--cuda-device-only", "-Rpass-analysis=kernel-resource-usage", "-c", "-o",
                                        os.devnull]
    err = subprocess.run(argv, cwd=pkg, check=True, capture_output=True, text=True).stderr
    filt = shutil.which("llvm-cxxfilt") or "c++filt"
    rows, cur = {}, None
    for ln in err.splitlines():
        m = re.search(r"remark: Function Name: (\S+)", ln)
        if m:
            cur = rows.setdefault(short_name(m.group(1), filt), {})
            continue
        m = re.search(r"remark:\s+(.+?): (\S+) \[-Rpass-analysis", ln)
        if m and cur is not None:
            cur[m.group(1)] = m.group(2)
    return rows


def natural(name):
    return [int(t) if t.isdigit() else t for t in re.split(r"(\d+)", name)]


def main():
    ap = argparse.ArgumentParser(description=__doc__.splitlines()[0])
    ap.add_argument("sources", nargs="+", help="csrc/*.hip files, relative to the package directory or absolute")
    ap.add_argument("--match", default="", help="print only the kernels whose name contains this text")
    ap.add_argument("--pkg", default=PKG, help="package directory holding the Makefile (default: this checkout's)")
    args = ap.parse_args()
    for src in args.sources:
        rows = resources(src, args.pkg)
        names = sorted((n for n in rows if args.match in n), key=natural)
        width = max([len(n) for n in names] + [36])
        print(f"# {src}")
        print(f"{'kernel':<{width}}  VGPR  AGPR  SGPR  scratch B/lane  waves/SIMD  LDS B/block")
        for n in names:
            r = rows[n]
            v = [r.get(k, "?") for k, _ in FIELDS]
            print(f"{n:<{width}}  {v[0]:>4}  {v[1]:>4}  {v[2]:>4}  {v[3]:>14}  {v[4]:>10}  {v[5]:>11}")
    return 0


if __name__ == "__main__":
    sys.exit(main())
