#!/usr/bin/env python3
"""Kernel-by-kernel comparison of the assembly hipcc -S writes for two versions of the same .hip files.

    for f in slp_cp_batch slp_cp_many slp_admm_many; do
      hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S OLD/pysparselp_amd/csrc/$f.hip -o old/$f.s
      hipcc <the Makefile's CXXFLAGS> --cuda-device-only -S     pysparselp_amd/csrc/$f.hip -o new/$f.s
    done
    python tools/lab/compare_isa.py old new [--rename 'REGEX=REPLACEMENT' ...] > profiles/NAME.txt

Kernels are matched by their demangled name (c++filt) up to the argument list, after the --rename rules were applied to
the OLD names.  A body is the text between the kernel's label and its .Lfunc_end, without comments and directives, the symbol
replaced and the local labels renumbered in order of appearance.  Two bodies are "identical" when they are the same text, and
"identical but for kernarg offsets" when the only differing lines are scalar loads from the kernarg segment whose immediate
offset moved (a parameter was added in front of the hidden arguments), and "same instructions, register numbers differ" when
they are the same text once every register number is masked (s12 -> s#, v[4:5] -> v[#+1]).  Otherwise the unified diff of the
masked bodies is printed, with the number of its changed lines that lie inside the iteration loop: the backward branch with
the longest span, in the new body.  Per kernel also the figures of its metadata comment block, before -> after."""
import difflib
import os
import re
import subprocess
import sys

FIGURES = (("NumVgprs", "vgprs"), ("TotalNumSgprs", "sgprs"), ("LDSByteSize", "lds"), ("ScratchSize", "scratch"), ("Occupancy", "occupancy"),
           ("codeLenInByte", "bytes"))


def kernels(path, cxxfilt):
    text = open(path).read()
    out = {}
    for m in re.finditer(r"^(_Z\w+):[^\n]*\n(.*?)^\.Lfunc_end\d+:\n(.*?)(?=-- Begin function|\Z)", text, re.S | re.M):
        sym, body, tail = m.groups()
        if ".amdhsa_kernel " + sym not in text:
            continue
        labels = {}
        lines = []
        for l in body.split("\n"):
            l = l.split(";")[0].rstrip()
            if not l.strip() or l.strip().startswith(".") and not l.strip().startswith(".LBB"):
                continue
            l = re.sub(r"\.LBB\d+_\d+", lambda g: labels.setdefault(g.group(0), ".L%d" % len(labels)), l.replace(sym, "KERNEL"))
            lines.append(l)
        fig = {}
        for key, name in FIGURES:
            g = re.search(r"; %s\s*[:=]\s*(\d+)" % key, tail)
            fig[name] = int(g.group(1)) if g else -1
        out[sym] = (lines, fig)
    names = subprocess.run([cxxfilt], input="\n".join(out), capture_output=True, text=True, check=True).stdout.split("\n")
    return {re.sub(r"^void ", "", n).split("(")[0]: v for n, v in zip(names, out.values())}


def only_kernarg_offsets(a, b):
    if len(a) != len(b):
        return False
    load = re.compile(r"^(\ts_load_\w+\s+\S+ s\[\d+:\d+\], )0x[0-9a-f]+$")
    return all(x == y or (load.match(x) and load.match(y) and load.match(x).group(1) == load.match(y).group(1)) for x, y in zip(a, b))


def masked(lines):
    wide = lambda g: "%s[#+%d]" % (g.group(1), int(g.group(3)) - int(g.group(2)))  # noqa: E731
    return [re.sub(r"\b([sv])\d+\b", r"\1#", re.sub(r"\b([sv])\[(\d+):(\d+)\]", wide, l)) for l in lines]


def iteration_loop(lines):
    """(first, last) line of the backward branch with the longest span, 1-based; (0, -1) without one."""
    at = {l[:-1]: i for i, l in enumerate(lines) if re.match(r"^\.L\d+:$", l)}
    best = (0, -1)
    for i, l in enumerate(lines):
        g = re.match(r"^\ts_c?branch\w*\s+(\.L\d+)$", l)
        if g and at.get(g.group(1), i) < i and i - at[g.group(1)] > best[1] - best[0]:
            best = (at[g.group(1)] + 1, i + 1)
    return best


def main():
    old_dir, new_dir = sys.argv[1], sys.argv[2]
    renames = [r.split("=", 1) for i, r in enumerate(sys.argv) if i > 2 and sys.argv[i - 1] == "--rename"]
    cxxfilt = os.environ.get("CXXFILT", "c++filt")
    counts = {}
    for f in sorted(os.listdir(new_dir)):
        old, new = kernels(os.path.join(old_dir, f), cxxfilt), kernels(os.path.join(new_dir, f), cxxfilt)
        for pat, to in renames:
            old = {re.sub(pat, to, k): v for k, v in old.items()}
        print("==== %s: %d kernels before, %d after" % (f, len(old), len(new)))
        for name in sorted(set(old) | set(new)):
            if name not in old or name not in new:
                print("%s\n    only %s" % (name, "before" if name in old else "after"))
                continue
            (a, fa), (b, fb) = old[name], new[name]
            verdict = ("identical" if a == b else "identical but for kernarg offsets" if only_kernarg_offsets(a, b) else
                       "same instructions, register numbers differ" if masked(a) == masked(b) else "DIFFERENT")
            counts[verdict] = counts.get(verdict, 0) + 1
            same = all(fa[k] == fb[k] for _, k in FIGURES[:5])
            print("%s\n    %s; %s%s" % (name, verdict, " ".join("%s %d -> %d" % (k, fa[k], fb[k]) for _, k in FIGURES),
                                        "" if same else "  <-- FIGURES CHANGED"))
            if verdict == "DIFFERENT":
                first, last = iteration_loop(b)
                inside = 0
                for l in difflib.unified_diff(masked(a), masked(b), "before", "after", n=0, lineterm=""):
                    print("        " + l)
                    g = re.match(r"^@@ -\S+ \+(\d+)(?:,(\d+))? @@", l)
                    if g:
                        lo, cnt = int(g.group(1)), int(g.group(2) or 1)
                        inside += sum(1 for x in range(lo, lo + max(cnt, 1)) if first <= x <= last)
                print("        %d changed lines inside the iteration loop, register numbers masked (lines %d-%d of %d)" % (inside, first, last, len(b)))
    print("==== " + ", ".join("%d %s" % (v, k) for k, v in sorted(counts.items())))


if __name__ == "__main__":
    main()
