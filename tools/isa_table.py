#!/usr/bin/env python3
"""Per-kernel table of a device assembly file (hipcc --cuda-device-only -S), or of two of them side by side.

    python tools/isa_table.py <file.s>                 one row per kernel
    python tools/isa_table.py <parent.s> <new.s>       both, with what differs

A row: kernel symbol, static instruction count, VGPRs, SGPRs, LDS bytes, scratch bytes, spilled VGPRs,
spilled SGPRs (the kernel's metadata), and a short hash of its instruction mix (the multiset of mnemonics, as
tools/isa_stats.py counts them).  With two files only the kernels that differ are listed:
    HARD   missing on one side, a metadata figure differs, or the new kernel spills VGPRs or uses scratch
    MIX    the metadata is equal and the instruction mix is not: its size and the mnemonics whose counts changed
    SSPILL equal on both sides, with SGPRs spilled (to VGPR lanes: no scratch) on both
and the exit status is 1 when there is a HARD row.
"""
import collections
import hashlib
import re
import sys

META = ("vgpr_count", "sgpr_count", "group_segment_fixed_size", "private_segment_fixed_size", "vgpr_spill_count",
        "sgpr_spill_count")


def kernels(path):
    text = open(path).read()
    meta = {}
    for blk in re.split(r"\n  - \.agpr_count:", text)[1:]:
        name = re.search(r"\.name:\s+(\S+)", blk)
        if name:
            meta[name.group(1)] = {k: int(re.search(rf"\.{k}:\s+(\d+)", blk).group(1)) for k in META}
    out = {}
    for m in re.finditer(r"^(_Z\S+):[^\n]*\n", text, re.M):
        name = m.group(1)
        if name not in meta:
            continue
        body = text[m.end():text.find(".Lfunc_end", m.end())]
        ins = [l.split()[0] for l in body.split("\n") if l.startswith("\t") and not l.startswith(("\t.", "\t;"))]
        out[name] = (collections.Counter(ins), meta[name])
    return out


def row(name, mix, meta):
    h = hashlib.sha256(repr(sorted(mix.items())).encode()).hexdigest()[:10]
    return f"{name}\t{sum(mix.values())}\t" + "\t".join(str(meta[k]) for k in META) + f"\t{h}"


def main(argv):
    a = kernels(argv[0])
    print("kernel\tinstructions\tvgpr\tsgpr\tlds\tscratch\tvgpr_spills\tsgpr_spills\tmix")
    if len(argv) == 1:
        for name, (mix, meta) in sorted(a.items()):
            print(row(name, mix, meta))
        return 0
    b = kernels(argv[1])
    hard = same = sspill = 0
    for name in sorted(set(a) | set(b)):
        if name not in a or name not in b:
            print(f"{name}\tONLY IN {'parent' if name in a else 'new'}")
            hard += 1
            continue
        (ma, ea), (mb, eb) = a[name], b[name]
        if ea != eb or eb["private_segment_fixed_size"] or eb["vgpr_spill_count"]:
            hard += 1
            print(f"HARD\t{row(name, ma, ea)}\n  ->\t{row(name, mb, eb)}")
        elif ma != mb:
            delta = {k: mb[k] - ma[k] for k in set(ma) | set(mb) if ma[k] != mb[k]}
            print(f"MIX\t{row(name, ma, ea)}\n  ->\t{row(name, mb, eb)}\t{sum(mb.values()) - sum(ma.values()):+d}\t"
                  + " ".join(f"{k}{v:+d}" for k, v in sorted(delta.items())))
        else:
            same += 1
            if eb["sgpr_spill_count"]:
                sspill += 1
                print(f"SSPILL\t{row(name, mb, eb)}")
    print(f"# {len(set(a) | set(b))} kernels: {same} identical in mix and metadata ({sspill} of them with SGPR spills on "
          f"both sides), {hard} hard differences")
    return 1 if hard else 0


if __name__ == "__main__":
    sys.exit(main(sys.argv[1:]))
