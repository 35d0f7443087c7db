#!/usr/bin/env python3
"""Which kernels of the library did a change to the sources touch?

    scripts/kernel_asm_diff.py OLD NEW [--rename 'old name=new name' ...]

OLD and NEW are source trees (checkouts of this repository) or device assembly files already emitted from them (*.s).
For a tree the device assembly of yag_slam_amd/csrc/yagmatch.hip is emitted with the library's own code generation flags.
Every kernel's instruction stream -- comments, blank lines, assembler directives and the numbers of local labels
stripped -- is compared between the two, and one line per kernel printed: "identical", or the two line counts.  A kernel
whose stream is identical runs the same code and needs no timing; one that differs does.  --rename pairs a kernel whose
(demangled) name changed.  Exit status 0.
"""
import argparse
import os
import re
import shutil
import subprocess
import sys
import tempfile

FLAGS = ["-O3", "-std=c++17", "--offload-arch=gfx950", "-ffp-contract=off", "-fno-fast-math", "--offload-device-only", "-S"]


def emit(path, tmp, tag):
    if os.path.isfile(path):
        return path
    src = os.path.join(path, "yag_slam_amd", "csrc")
    out = os.path.join(tmp, tag + ".s")
    hipcc = os.environ.get("HIPCC", "/opt/rocm/bin/hipcc")
    subprocess.run([hipcc] + FLAGS + ["yagmatch.hip", "-o", out], cwd=src, check=True)
    return out


def demangle(names):
    tool = shutil.which("c++filt") or shutil.which("llvm-cxxfilt")
    if not tool:
        return {n: n for n in names}
    out = subprocess.run([tool], input="\n".join(names), capture_output=True, text=True, check=True).stdout.split("\n")
    short = {}
    for n, d in zip(names, out):
        d = re.sub(r"^void ", "", d)
        short[n] = re.sub(r"\((?:[^()]|\([^()]*\))*\)$", "", d)  # without the parameter list
    return short


def kernels(asm_path):
    """demangled kernel name -> list of normalised instruction lines"""
    lines = open(asm_path).read().split("\n")
    names = [l.split()[1] for l in lines if l.strip().startswith(".amdhsa_kernel ")]
    start = {}
    for i, l in enumerate(lines):
        head = l.split(";")[0].rstrip()
        if head.endswith(":") and not head.startswith((".", " ", "\t")):
            start.setdefault(head[:-1], i)
    short = demangle(names)
    streams = {}
    for n in names:
        body = []
        for l in lines[start[n] + 1:]:
            if l.startswith(".Lfunc_end"):
                break
            l = l.split(";")[0].strip()
            if not l or (l.startswith(".") and not l.endswith(":")):
                continue  # a directive; labels stay, as the places branches go to
            body.append(re.sub(r"\.L([A-Za-z]+)\d+_", r".L\1_", l))
        streams[short[n]] = body
    return streams


def main():
    ap = argparse.ArgumentParser(description=__doc__, formatter_class=argparse.RawDescriptionHelpFormatter)
    ap.add_argument("old")
    ap.add_argument("new")
    ap.add_argument("--rename", action="append", default=[], metavar="OLD=NEW")
    args = ap.parse_args()
    renamed = dict(r.split("=", 1) for r in args.rename)
    with tempfile.TemporaryDirectory() as tmp:
        old = kernels(emit(args.old, tmp, "old"))
        new = kernels(emit(args.new, tmp, "new"))
    same = differ = 0
    for name in sorted(old):
        to = renamed.get(name, name)
        label = name if to == name else "%s -> %s" % (name, to)
        if to not in new:
            print("%-90s only in OLD (%d lines)" % (label, len(old[name])))
        elif old[name] == new[to]:
            same += 1
            print("%-90s identical" % label)
        else:
            differ += 1
            print("%-90s DIFFERS: %d lines -> %d lines" % (label, len(old[name]), len(new[to])))
    for name in sorted(set(new) - {renamed.get(n, n) for n in old}):
        print("%-90s only in NEW (%d lines)" % (name, len(new[name])))
    print("%d kernels identical, %d differ" % (same, differ), file=sys.stderr)


if __name__ == "__main__":
    main()
