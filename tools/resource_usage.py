#!/usr/bin/env python3
"""Kernel resource tables from hipcc's -Rpass-analysis=kernel-resource-usage.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only \\
          -Rpass-analysis=kernel-resource-usage -c cilium_amd/csrc/kernels.hip \\
          -o /dev/null 2> remarks.txt
    python tools/resource_usage.py table remarks.txt > usage.tsv
    python tools/resource_usage.py diff parent.tsv branch.tsv

`table` prints one line per kernel of the project (name and template
arguments; library kernels such as rocprim's are left out): SGPRs, VGPRs,
AGPRs, scratch bytes per lane, occupancy in waves per SIMD, spills, static
LDS.  `diff` compares two tables by kernel name, matching a kernel whose
template arguments a change appended to (all appended ones `false`) with the
name it had before, and exits 1 when a kernel of the first table is missing
from the second or differs in any column.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -I include --cuda-device-only \\
          -S cilium_amd/csrc/kernels.hip -o branch.s
    python tools/resource_usage.py isa parent.s branch.s

`isa` compares two assembly listings function by function (kernels and the
device functions left out of line), ignoring comments, debug lines and the
numbers in compiler-local labels, which renumber when an earlier function
goes; it names the functions that differ or exist on one side only and exits
1 when one differs.  (Assembly, not linked objects: those differ in
pc-relative literals once anything moves.)
"""
import re
import subprocess
import sys

COLS = ("TotalSGPRs", "VGPRs", "AGPRs", "ScratchSize [bytes/lane]", "Occupancy [waves/SIMD]",
        "SGPRs Spill", "VGPRs Spill", "LDS Size [bytes/block]")


def parse(path):
    rows, cur = {}, None
    for line in open(path, errors="replace"):
        m = re.search(r"remark:\s+(.*?) \[-Rpass-analysis", line)
        if not m:
            continue
        k, _, v = m.group(1).partition(": ")
        k = k.strip()
        if k == "Function Name":
            cur = rows.setdefault(v.strip(), {})
        elif cur is not None and k in COLS:
            cur[k] = v.strip()
    return rows


def demangle(names):
    try:
        out = subprocess.run(["c++filt"], input="\n".join(names), capture_output=True, text=True,
                             check=True).stdout.splitlines()
        return dict(zip(names, out))
    except (OSError, subprocess.CalledProcessError):
        return {n: n for n in names}


def table(path):
    rows = parse(path)
    dm = demangle(list(rows))
    print("\t".join(("kernel",) + COLS))
    for n in sorted(rows, key=lambda x: dm[x]):
        k, targs, _ = base(dm[n].replace("(anonymous namespace)::", ""))
        if "::" in k:
            continue  # a library's kernel (rocprim's sort), not built from this source
        print("\t".join([k + ("<" + ", ".join(targs) + ">" if targs else "")] + [rows[n].get(c, "") for c in COLS]))


def load(path):
    out = {}
    for line in open(path).read().splitlines()[1:]:
        f = line.split("\t")
        out[f[0]] = f[1:]
    return out


def base(name):
    """void k<a, b, c>(x, y) -> ('k', [a, b, c], [x, y])"""
    m = re.match(r"(?:void )?([\w:]+)(?:<(.*)>)?(?:\((.*)\))?$", name)
    if not m:
        return name, [], []

    def split(s):
        parts, depth, cur = [], 0, ""
        for ch in s or "":
            depth += ch in "<("
            depth -= ch in ">)"
            if ch == "," and depth == 0:
                parts.append(cur.strip())
                cur = ""
            else:
                cur += ch
        return parts + ([cur.strip()] if cur.strip() else [])
    return m.group(1), split(m.group(2)), split(m.group(3))


def diff(pa, pb):
    a, b = load(pa), load(pb)
    bad = same = 0
    matched = set()
    for na, ra in sorted(a.items()):
        ka, ta, fa = base(na)
        match = None
        for nb in b:
            kb, tb, fb = base(nb)
            # the branch's kernel of this name: equal leading arguments, any
            # appended template arguments false (the feature off)
            if kb == ka and tb[:len(ta)] == ta and fb[:len(fa)] == fa and \
                    all(x == "false" for x in tb[len(ta):]):
                match = nb
                break
        if match is None:
            print(f"ONLY IN {pa}: {na}")
            bad += 1
            continue
        matched.add(match)
        if b[match] != ra:
            print(f"DIFFERS: {na}\n  {pa}: {ra}\n  {pb}: {b[match]}")
            bad += 1
        else:
            same += 1
    print(f"{same} kernels equal in every column, {bad} differing or missing; "
          f"{len(b) - len(matched)} only in {pb}")
    return 1 if bad else 0


def functions(path):
    """{symbol: its assembly from .type to .Lfunc_end and the .size / .set
    lines behind it}, without comments, .loc / .file lines and the numbers of
    compiler-local labels"""
    out, cur, ending = {}, None, False
    for line in open(path, errors="replace"):
        line = line.split(";", 1)[0].rstrip()
        m = re.match(r"\s*\.type\s+(\S+),@function", line)
        if m:
            cur, ending = out.setdefault(m.group(1), []), False
        if cur is None or not line.strip() or re.match(r"\s*\.(loc|file)\s", line):
            continue
        if ending and not re.match(r"\s*\.(size|set)\s", line):
            cur = None
            continue
        ending = ending or re.match(r"\.Lfunc_end\d+:", line) is not None
        cur.append(re.sub(r"\.(LBB|Ltmp|LJTI|Lfunc_begin|Lfunc_end)\d+", r".\1", line))
    return out


def isa(pa, pb):
    a, b = functions(pa), functions(pb)
    dm = demangle(sorted(set(a) | set(b)))
    differ = [n for n in a if n in b and a[n] != b[n]]
    for n in sorted(differ, key=dm.get):
        print(f"DIFFERS: {dm[n]}")
    for path, x, y in ((pa, a, b), (pb, b, a)):
        for n in sorted(set(x) - set(y), key=dm.get):
            print(f"ONLY IN {path}: {dm[n]}")
    print(f"{len(set(a) & set(b)) - len(differ)} functions identical, {len(differ)} differing; "
          f"{len(set(a) - set(b))} only in {pa}, {len(set(b) - set(a))} only in {pb}")
    return 1 if differ else 0


if __name__ == "__main__":
    if len(sys.argv) == 3 and sys.argv[1] == "table":
        table(sys.argv[2])
    elif len(sys.argv) == 4 and sys.argv[1] == "diff":
        sys.exit(diff(sys.argv[2], sys.argv[3]))
    elif len(sys.argv) == 4 and sys.argv[1] == "isa":
        sys.exit(isa(sys.argv[2], sys.argv[3]))
    else:
        sys.exit(__doc__)
