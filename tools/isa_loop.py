#!/usr/bin/env python3
"""Instruction mix of the loops of one kernel in a device assembly file: for every loop header
label, the static instruction counts of the blocks that the compiler's comments put in that loop
(`=>This Inner Loop Header`, `in Loop: Header=BBn_m`), whichever way its back edge enters.

    python tools/isa_loop.py <file.s> <symbol-substring> [max-loops] [--barriers]

--barriers: only loops that hold an s_barrier (the iteration loops of the flood kernels).
"""
import collections
import re
import sys


def loops(body):
    """-> {header label: Counter of opcodes}, in order of appearance"""
    per, tag = collections.OrderedDict(), None
    for l in body:
        m = re.match(r"(\.LBB\d+_\d+|; %bb\.\d+):(.*)", l)
        if m:
            h = re.search(r"Header=(BB\d+_\d+)", m.group(2))
            if "Loop Header" in m.group(2) and m.group(1).startswith(".L"):
                tag = m.group(1)[2:]
            else:
                tag = h.group(1) if h else None
            if tag:
                per.setdefault(tag, collections.Counter())
            continue
        if tag and l.startswith("\t") and not l.startswith("\t.") and not l.startswith("\t;"):
            per[tag][l.split()[0]] += 1
    return per


def main(path, sub, nmax=4, *flags):
    s = open(path).read()
    m = next(m for m in re.finditer(r"^(_Z\S+):[^\n]*\n", s, re.M) if sub in m.group(1))
    per = loops(s[m.end():s.index(".Lfunc_end", m.end())].split("\n"))
    if "--barriers" in flags:
        per = collections.OrderedDict((k, c) for k, c in per.items() if c.get("s_barrier"))
    print(m.group(1), len(per), "loops")
    for lab, c in list(per.items())[:int(nmax)]:
        n = lambda p: sum(k for i, k in c.items() if i.startswith(p))
        print(f"-- .L{lab}: {sum(c.values())} instructions, VALU {n('v_')}, v_mov {n('v_mov')}, LDS {n('ds_')}, "
              f"s_waitcnt {c['s_waitcnt']}, branches {n('s_cbranch') + n('s_branch')}, s_nop {c['s_nop']}, "
              f"global_store {n('global_store')}, global_atomic {n('global_atomic')}")
        print("   " + ", ".join(f"{i} {k}" for i, k in c.most_common(28)))


if __name__ == "__main__":
    main(*sys.argv[1:])
