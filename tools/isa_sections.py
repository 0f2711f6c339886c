#!/usr/bin/env python3
"""Static instruction counts of one kernel, per barrier-delimited section, from an ISA listing.

  hipcc -O3 -fPIC --offload-arch=gfx950 -std=c++17 --cuda-device-only -S \
        -o dmx_kernels.s deflate_compression_amd/csrc/dmx_kernels.hip
  python3 tools/isa_sections.py dmx_kernels.s _Z16dmx_match_kernelILb0ELi3ELb0EEv9MatchArgs

A section is the code between two s_barrier instructions in listing order (which is the
execution order of straight-line code; loops and branches are counted once, as listed).
Per section: vector ALU instructions (v_*, without v_readlane/v_writelane spill traffic
listed apart), LDS instructions (ds_*), exec-mask branches (s_cbranch_execz/execnz) and the
mnemonics that identify the section.  With --marks only sections holding one of the given
mnemonics are printed (e.g. --marks v_sad_u8,v_pk_sub_u16,ds_write_b16).
"""
import argparse
import collections
import re


def kernel_body(path, name):
    out, on = [], False
    for line in open(path):
        if line.startswith(name + ":"):
            on = True
            continue
        if on:
            if line.startswith(".Lfunc_end"):
                break
            out.append(line)
    if not out:
        raise SystemExit(f"kernel {name} not found in {path}")
    return out


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("listing")
    ap.add_argument("kernel")
    ap.add_argument("--marks", default="")
    ap.add_argument("--top", type=int, default=6, help="most frequent mnemonics shown per section")
    a = ap.parse_args()
    marks = [m for m in a.marks.split(",") if m]
    secs = [collections.Counter()]
    for line in kernel_body(a.listing, a.kernel):
        m = re.match(r"\s+([a-z][a-z0-9_]+)\b", line)
        if not m:
            continue
        op = m.group(1)
        if op == "s_barrier":
            secs.append(collections.Counter())
        else:
            secs[-1][op] += 1
    print(f"{'sec':>4} {'valu':>6} {'lane':>5} {'ds':>5} {'exbr':>5} {'all':>6}  mnemonics")
    tv = 0
    for i, c in enumerate(secs):
        lane = sum(n for op, n in c.items() if op.startswith(("v_readlane", "v_writelane", "v_readfirstlane")))
        valu = sum(n for op, n in c.items() if op.startswith("v_")) - lane
        ds = sum(n for op, n in c.items() if op.startswith("ds_"))
        br = sum(n for op, n in c.items() if op.startswith("s_cbranch_exec"))
        tv += valu + lane
        if marks and not any(c[m] for m in marks):
            continue
        top = " ".join(f"{op}:{n}" for op, n in c.most_common(a.top))
        mk = " ".join(f"[{m}:{c[m]}]" for m in marks if c[m])
        print(f"{i:>4} {valu:>6} {lane:>5} {ds:>5} {br:>5} {sum(c.values()):>6}  {mk} {top}")
    print(f"vector instructions listed in the kernel: {tv}")


if __name__ == "__main__":
    main()
