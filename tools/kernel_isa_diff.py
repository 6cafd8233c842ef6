#!/usr/bin/env python3
"""Compare the kernels of two directories of device assembly (`make -C
minibase-columnar-database_amd/csrc asm ASMDIR=...` before and after a change):

    tools/kernel_isa_diff.py OLD_DIR NEW_DIR [--quiet]

A kernel is SAME when every copy of it in NEW_DIR has the instruction stream
and the .amdhsa_* descriptor of its copy in OLD_DIR, comments dropped and
basic-block label numbers ignored.  Prints one line per kernel symbol with the
files that hold it, then the added and missing symbols; exit status 1 unless
every symbol is SAME and none is added or missing."""
import glob
import os
import re
import sys

LABEL = re.compile(r"\.L(BB|func_end|func_begin|tmp)\d+")


def kernels(directory):
    """symbol -> {file: (instruction lines, descriptor lines)}"""
    out = {}
    for path in sorted(glob.glob(os.path.join(directory, "*.s"))):
        lines = [l.split(";")[0].rstrip() for l in open(path)]
        lines = [LABEL.sub(lambda m: ".L" + m.group(1), l) for l in lines if l.strip()]
        body = {}
        for i, l in enumerate(lines):
            if l.endswith(":") and not l.startswith((".", " ", "\t")):
                end = next((j for j in range(i, len(lines)) if lines[j].startswith(".Lfunc_end")), None)
                if end is not None:  # a function, not a data symbol behind the last one
                    body[l[:-1]] = lines[i + 1:end]
        for i, l in enumerate(lines):
            if l.strip().startswith(".amdhsa_kernel "):
                sym = l.split()[1]
                end = lines.index("\t.end_amdhsa_kernel", i)
                out.setdefault(sym, {})[os.path.basename(path)] = (body[sym], lines[i + 1:end])
    return out


def main():
    args = [a for a in sys.argv[1:] if a != "--quiet"]
    quiet = len(args) != len(sys.argv) - 1
    old, new = kernels(args[0]), kernels(args[1])
    same = 0
    for sym in sorted(old):
        if sym not in new:
            continue
        ref = next(iter(old[sym].values()))
        ok = all(copy == ref for copy in list(old[sym].values()) + list(new[sym].values()))
        same += ok
        if not (ok and quiet):
            print("SAME" if ok else "DIFF", sym, ",".join(old[sym]), "->", ",".join(new[sym]))
    added, missing = sorted(set(new) - set(old)), sorted(set(old) - set(new))
    for sym in added:
        print("ADDED", sym, ",".join(new[sym]))
    for sym in missing:
        print("MISSING", sym, ",".join(old[sym]))
    print(f"{len(old)} kernels before, {len(new)} after: {same} identical, "
          f"{len(old) - len(missing) - same} differ, {len(added)} added, {len(missing)} missing")
    return 0 if same == len(old) == len(new) else 1


if __name__ == "__main__":
    sys.exit(main())
