#!/usr/bin/env python3
"""Per-symbol comparison of the kernels' assembly of two trees (`make -C phosphorus_mk2_amd/csrc asm` on both): which kernels' instruction
streams differ, with basic-block labels renumbered by first appearance and comments, debug and CFI directives dropped.  Each side is one .s
file, several joined by commas, or a directory of them (one .s per kernel family: trace.s, shade_lambert.s, shade_general.s, film_hooks.s):

    python scripts/asm_compare.py PARENT/phosphorus_mk2_amd/csrc phosphorus_mk2_amd/csrc
"""
import os
import re
import subprocess
import sys


def files_of(side):
    """a side of the comparison: one .s file, several joined by commas, or a directory (every .s file in it)"""
    paths = []
    for p in side.split(","):
        paths += sorted(os.path.join(p, f) for f in os.listdir(p) if f.endswith(".s")) if os.path.isdir(p) else [p]
    return paths


def bodies(side):
    """symbol -> its lines up to .Lfunc_end, comments stripped, over all files of the side"""
    out = {}
    for path in files_of(side):
        for name, lines in bodies_of_file(path).items():
            if name in out and renumbered(out[name]) != renumbered(lines):
                sys.exit(f"{name} is defined with different bodies in two files of {side}")
            out[name] = lines
    return out


def bodies_of_file(path):
    out, cur = {}, None
    for line in open(path):
        m = re.match(r"^(_Z\w+|[A-Za-z_]\w*):\s*(;.*)?$", line)
        if m:
            cur = None if m.group(1).startswith("__hip_cuid") else m.group(1)  # (the build's id symbol: data, and the file's metadata behind it)
            if cur:
                out[cur] = []
            continue
        if cur is None:
            continue
        if line.lstrip().startswith(".Lfunc_end"):
            cur = None
            continue
        s = line.split(";")[0].strip()
        if s and not s.startswith((".loc", ".cfi", ".file")):
            out[cur].append(s)
    return out


def renumbered(lines):
    seen = {}
    return [re.sub(r"\.LBB\d+_\d+", lambda x: seen.setdefault(x.group(0), f".L{len(seen)}"), l) for l in lines]


def main():
    a, b = bodies(sys.argv[1]), bodies(sys.argv[2])
    names = sorted(set(a) | set(b))
    plain = dict(zip(names, subprocess.run(["c++filt"] + names, capture_output=True, text=True).stdout.splitlines()))
    both = [n for n in names if n in a and n in b]
    changed = [n for n in both if renumbered(a[n]) != renumbered(b[n])]
    new, gone = [n for n in names if n not in a], [n for n in names if n not in b]
    print(f"symbols: {len(names)}; identical instruction for instruction (basic-block labels renumbered): {len(both) - len(changed)}; "
          f"changed: {len(changed)}; new: {len(new)}; gone: {len(gone)}")
    for n in changed:
        print(f"changed  {re.sub(r'[(]phx::DevScene.*', '', plain[n]):70s} {len(a[n]):6d} -> {len(b[n]):6d} lines")
    for n in new:
        print("new     ", plain[n])
    for n in gone:
        print("gone    ", plain[n])


if __name__ == "__main__":
    main()
