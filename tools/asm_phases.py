#!/usr/bin/env python3
"""Static instruction counts of k_decode_idx by phase, from a
-gline-tables-only device assembly:

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -Iinclude -Ibo-lz4-ada_amd/csrc \
        -mllvm -amdgpu-sched-strategy=iterative-ilp -gline-tables-only -S \
        --cuda-device-only -o /tmp/idxg.s bo-lz4-ada_amd/csrc/lz4ada_idx.hip
    python tools/asm_phases.py /tmp/idxg.s

An instruction belongs to the call-site line inside decode_block or
index_block that its .loc's inline chain leads to.  The phases are the
stretches between the ISTAMP() marks of those two functions, read from the
source (lz4ada_idx.hip and the part it includes, lz4ada_idx_pass1.inc), so
they follow the files as they change: pass 1's stage / lead-in / first walk /
re-walk / table write (index_block) and pass 2's phases (decode_block),
named as tools/idx_stamps.py names their cycles."""
import collections
import os
import re
import sys

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "bo-lz4-ada_amd", "csrc")
UNIT, PASS1 = "lz4ada_idx.hip", "lz4ada_idx_pass1.inc"
P1_NAMES = {"I_STAGE": "p1 stage", "I_LEAD": "p1 lead-in", "I_WALK0": "p1 first walk",
            "I_ITER": "p1 re-walk"}


def func_range(src, name):
    """(first, last) 1-based lines of the definition of `name`: from its
    header to the closing brace in column 0."""
    a = next(i for i, l in enumerate(src) if re.match(r"^__(device|global)__ .*\b%s\(" % name, l))
    b = next(i for i in range(a, len(src)) if src[i].startswith("}"))
    return a + 1, b + 1


def phases(srcs):
    """[(file, first line, last line, name)] of index_block and decode_block."""
    ph = []
    for f, fn, tail, names in ((PASS1, "index_block", "p1 table write", P1_NAMES), (UNIT, "decode_block", "end", {})):
        src = srcs[f]
        a, b = func_range(src, fn)
        cur = a
        for i in range(a, b + 1):
            m = re.search(r"\bISTAMP\((\w+)\)", src[i - 1])
            if m:
                ph.append((f, cur, i, names.get(m.group(1), m.group(1))))
                cur = i + 1
        ph.append((f, cur, b, tail))
    return ph


def main():
    srcs = {f: open(os.path.join(CSRC, f)).read().split("\n") for f in (UNIT, PASS1)}
    ph = phases(srcs)
    kern = func_range(srcs[UNIT], "k_decode_idx")

    def phase(loc):
        for f, a, b, n in ph:
            if f == loc[0] and a <= loc[1] <= b:
                return n
        return "other:%s:%d" % loc

    lines = open(sys.argv[1]).read().split("\n")
    start = next(i for i, l in enumerate(lines) if re.match(r"^_ZN6lz4ada3idx12k_decode_idxE\w*:", l))
    cnt = collections.defaultdict(collections.Counter)
    cur = "none"
    for l in lines[start:]:
        if l.startswith(".Lfunc_end"):
            break
        m = re.match(r"\s*\.loc\s+\d+\s+\d+.*?;\s*(.*)$", l)
        if m:
            chain = [(f, int(x)) for f, x in re.findall(r"(lz4ada_idx\w*\.\w+):(\d+)", m.group(1))]
            inner = [c for c in chain if not (c[0] == UNIT and kern[0] <= c[1] <= kern[1])]
            cur = phase(inner[-1]) if inner else "kernel"
            continue
        s = l.strip()
        if not s or s.startswith((".", ";")) or s.endswith(":"):
            continue
        op = s.split()[0]
        c = cnt[cur]
        c["all"] += 1
        if op.startswith("v_"):
            c["valu"] += 1
        elif op.startswith(("s_cbranch", "s_branch")):
            c["br"] += 1
        elif op.startswith("s_waitcnt") or op.startswith("s_nop"):
            c["wait"] += 1
        elif op.startswith("s_"):
            c["salu"] += 1
        elif op.startswith("ds_"):
            c["lds"] += 1
        elif op.startswith(("global_", "buffer_", "flat_")):
            c["vmem"] += 1
    for k, c in sorted(cnt.items(), key=lambda kv: -kv[1]["all"]):
        print(f"{k:16s} {c['all']:6d} v{c['valu']:5d} s{c['salu']:5d} br{c['br']:4d} w{c['wait']:4d} "
              f"lds{c['lds']:4d} vm{c['vmem']:4d}")


if __name__ == "__main__":
    main()
