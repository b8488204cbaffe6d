#!/usr/bin/env python3
"""The order of a kernel's memory instructions and waits, from its assembly.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only \\
          -S cilium_amd/csrc/kernels.hip -o kernels.s
    python tools/loop_waits.py kernels.s 'k_classify_x4<1024, true, 4, 1, false, false, 0, false, false, false>'

Prints, for the kernel whose demangled name contains the second argument,
every vector memory instruction (loads, stores, atomics), every `s_waitcnt`
that waits on vmcnt, and the labels and branches between them, each with its
line number in the kernel.  Loads that are in flight together show as
consecutive load lines with no wait between them; a load that is waited for
before the next one is issued shows as load, wait, load, wait.
"""
import re
import subprocess
import sys

KEEP = re.compile(r"^\s*(global_|buffer_|flat_|scratch_)(load|store|atomic)|^\s*s_waitcnt.*vmcnt|"
                  r"^\s*s_c?branch|^\.LBB\w+:")


def kernels(lines):
    """{mangled name: (first line, last line)} of the file's functions"""
    out, cur = {}, None
    for i, l in enumerate(lines):
        m = re.match(r"^(\w+):", l)
        if m and not l.startswith(".L") and f"\t.type\t{m.group(1)},@function" in "".join(lines[max(0, i - 8):i]):
            cur = (m.group(1), i)
        elif l.startswith(".Lfunc_end") and cur:
            out[cur[0]] = (cur[1], i)
            cur = None
    return out


def main(path, want):
    lines = open(path, errors="replace").read().splitlines(keepends=True)
    ks = kernels(lines)
    names = list(ks)
    dm = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                        check=True).stdout.splitlines()
    hits = [n for n, d in zip(names, dm) if want in d.replace("(anonymous namespace)::", "")]
    if len(hits) != 1:
        sys.exit(f"{len(hits)} kernels match {want!r}")
    a, b = ks[hits[0]]
    print(f"# {dict(zip(names, dm))[hits[0]]}")
    for i in range(a, b):
        l = lines[i].split(";")[0].rstrip()
        if KEEP.match(l):
            print(f"{i - a:6d}  {l.strip()}")


if __name__ == "__main__":
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    main(sys.argv[1], sys.argv[2])
