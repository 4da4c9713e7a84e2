#!/usr/bin/env python3
"""Static instruction counts of a kernel's main loop, from the assembly hipcc -S writes.

    hipcc --offload-arch=gfx950 -O3 -std=c++17 -ffp-contract=off -mllvm -amdgpu-sched-strategy=max-ilp \
          --cuda-device-only -S pysparselp_amd/csrc/slp_tall_spmv.hip -o tall.s
    python tools/lab/count_loop.py tall.s k_tall_spmvILb1ELb0ELb0ELi4096E

The main loop is found by the compiler's own loop annotations of the basic blocks (blocks the layout moved behind the loop
included): the largest loop that holds no inner loop of half its size (the loop over segments is around the packet loop).
Classes: vector (v_*), scalar (s_*; scalar_alu leaves out waits, barriers, nops and branches), LDS (ds_*), vector memory
(buffer_*, global_*, flat_*, scratch_*).  Also prints the
kernel's register and scratch figures from its metadata comment block."""
import re
import sys


def main():
    path, key = sys.argv[1], sys.argv[2]
    lines = open(path).read().split("\n")
    # (the symbol's own label line "<mangled name>:", whatever the kernel's argument list mangles to)
    start = next(i for i, l in enumerate(lines) if l.startswith("_ZN") and key in l.split(":")[0] and ":" in l)
    end = next(i for i in range(start, len(lines)) if lines[i].strip().startswith("s_endpgm"))
    # every basic block carries the compiler's loop annotation ("in Loop: Header=BBn_m Depth=d"; the header itself "Parent Loop"
    # / "This ... Loop Header" on its own line and the next): the main loop is the innermost-or-not loop with the most instructions
    # that holds no inner loop of half its size -- the segment loop around the packet loop does
    blocks, cur, hdr_of = {}, None, {}
    i = start
    while i < end:
        l = lines[i]
        m = re.match(r"^(?:\.L(BB\d+_\d+):|; %bb\.(\d+):)\s*(;.*)?$", l)
        if m:
            name = m.group(1) or "bb." + m.group(2)
            note = (m.group(3) or "") + " " + (lines[i + 1] if lines[i + 1].lstrip().startswith(";") and "Loop" in lines[i + 1] else "")
            hdrs = re.findall(r"Header=(BB\d+_\d+)", note)
            if "Loop Header" in note:
                hdrs, depth = [name], int(re.search(r"Loop Header: Depth=(\d+)", note).group(1))
                parents = re.findall(r"Parent Loop (BB\d+_\d+)", note)
                hdr_of[name] = parents[-1] if parents else None
            cur = hdrs[0] if hdrs else None
        elif cur and re.match(r"^\s+[a-z_0-9]+(\s|$)", l):
            blocks.setdefault(cur, []).append(i)
        i += 1
    def whole(h):   # a loop's own blocks and those of the loops inside it
        return blocks.get(h, []) + [j for c, par in hdr_of.items() if par == h for j in whole(c)]
    sizes = {h: len(whole(h)) for h in set(blocks) | set(hdr_of)}
    main_hdr = max((h for h in sizes if not any(par == h and 2 * sizes[c] >= sizes[h] for c, par in hdr_of.items())), key=lambda h: sizes[h])
    body = sorted(whole(main_hdr))
    cnt = {"vector": 0, "scalar": 0, "lds": 0, "vmem": 0, "other": 0}
    detail = {}
    for i in body:
        m = re.match(r"^\s+([a-z_0-9]+)(\s|$)", lines[i])
        op = m.group(1)
        k = ("vector" if op.startswith("v_") else "scalar" if op.startswith("s_") else "lds" if op.startswith("ds_")
             else "vmem" if op.split("_")[0] in ("buffer", "global", "flat", "scratch") else "other")
        cnt[k] += 1
        detail[op] = detail.get(op, 0) + 1
    cnt["scalar_alu"] = cnt["scalar"] - sum(n for op, n in detail.items() if op in ("s_waitcnt", "s_barrier", "s_nop", "s_branch") or op.startswith("s_cbranch"))
    print("loop with header %s: %d instructions" % (main_hdr, len(body)), cnt)
    if len(sys.argv) > 3:
        for op, n in sorted(detail.items(), key=lambda t: -t[1]):
            print("  %-28s %d" % (op, n))
    for i in range(end, min(end + 200, len(lines))):
        if re.search(r"; (NumSgprs|NumVgprs|ScratchSize|Occupancy|sgpr_spill_count|vgpr_spill_count|SGPRBlocks|NumAgprs|TotalNumVgprs)\b", lines[i]) or \
           re.search(r"\.(sgpr|vgpr)_spill_count|\.private_segment_fixed_size", lines[i]):
            print(lines[i].strip())


if __name__ == "__main__":
    main()
