#!/usr/bin/env python3
"""Compare the device code of two builds kernel by kernel.

    make -C genome.distance_amd asm          # in each tree: build/asm/<name>.s
    scripts/kernel_isa_diff.py DIR_A DIR_B

Reads every .s file of the two directories, splits them by kernel symbol
(a function that has an .amdhsa_kernel descriptor) and compares, per symbol,
the normalised body and the descriptor block. Which file a kernel sits in
does not matter: a kernel that moved to another source compares equal as long
as its instructions and its descriptor are the same. Normalisation: label
numbers (.LBB<n>_, .Lfunc_*<n>, .Ltmp<n>) are renumbered away, comments and
whitespace dropped, .section / .text lines ignored.

Prints the counts (kernels in A, in B, identical, differing, on one side
only) and names every kernel that is not identical. Exit status 0 only when
both sides hold the same kernels and none differs.
"""
import glob
import os
import re
import sys

LABEL = re.compile(r"^([A-Za-z_.$][\w.$]*):")
KERNEL = re.compile(r"^\.amdhsa_kernel\s+(\S+)")
FUNC_END = re.compile(r"^\.Lfunc_end\d+:")


def normalise(lines):
    """Body lines -> comparable lines (see the module docstring)."""
    tmp = {}

    def ltmp(m):
        return ".Ltmp#%d" % tmp.setdefault(m.group(0), len(tmp))

    out = []
    for line in lines:
        line = line.split(";", 1)[0] if '"' not in line else line
        line = " ".join(line.split())
        if not line or line.startswith((".section", ".text")):
            continue
        line = re.sub(r"\.LBB\d+_", ".LBB_", line)
        line = re.sub(r"\.Lfunc_(begin|end)\d+", r".Lfunc_\1", line)
        line = re.sub(r"\.Ltmp\d+", ltmp, line)
        out.append(line)
    return out


def kernels_of(path):
    """{symbol: (body lines, descriptor lines)} of one .s file."""
    with open(path, errors="replace") as f:
        text = [ln.rstrip("\n") for ln in f]
    found = {}
    i = 0
    while i < len(text):
        m = LABEL.match(text[i])
        if not m or m.group(1).startswith(".L"):
            i += 1
            continue
        sym, body, desc, in_desc, is_kernel = m.group(1), [], [], False, False
        j = i + 1
        while j < len(text) and not FUNC_END.match(text[j].strip()):
            s = text[j].strip()
            if LABEL.match(text[j]) and not text[j].startswith(".L"):
                break                                  # a data symbol, not a function: no .Lfunc_end of its own
            k = KERNEL.match(s)
            if k:
                in_desc, is_kernel = True, k.group(1) == sym
            (desc if in_desc else body).append(text[j])
            if s.startswith(".end_amdhsa_kernel"):
                in_desc = False
            j += 1
        if is_kernel and j < len(text) and FUNC_END.match(text[j].strip()):
            found[sym] = (normalise(body), normalise(desc))
        i = j + 1 if j > i else i + 1
    return found


def kernels_in(directory):
    files = sorted(glob.glob(os.path.join(directory, "*.s")))
    if not files:
        sys.exit(f"{directory}: no .s files (run `make -C genome.distance_amd asm`)")
    found = {}
    for path in files:
        for sym, k in kernels_of(path).items():
            if sym in found and found[sym][:2] != k:
                print(f"note: {sym} is defined differently in two files of {directory}")
            found[sym] = k + (os.path.basename(path),)
    return found


def main():
    if len(sys.argv) != 3:
        sys.exit(__doc__)
    a, b = kernels_in(sys.argv[1]), kernels_in(sys.argv[2])
    only_a, only_b = sorted(set(a) - set(b)), sorted(set(b) - set(a))
    both = sorted(set(a) & set(b))
    differing = [s for s in both if a[s][:2] != b[s][:2]]
    moved = [s for s in both if a[s][2] != b[s][2] and s not in differing]
    print(f"A: {sys.argv[1]}\nB: {sys.argv[2]}")
    print(f"kernels in A: {len(a)}\nkernels in B: {len(b)}")
    print(f"identical: {len(both) - len(differing)} (of them in another file in B: {len(moved)})")
    print(f"differing: {len(differing)}\nonly in A: {len(only_a)}\nonly in B: {len(only_b)}")
    print(f"normalised lines compared: {sum(len(a[s][0]) + len(a[s][1]) for s in both)}")
    for title, names in (("differing", differing), ("only in A", only_a), ("only in B", only_b)):
        for s in names:
            where = a[s][2] if s in a else b[s][2]
            print(f"{title}: {s} ({where})")
    sys.exit(1 if differing or only_a or only_b else 0)


if __name__ == "__main__":
    main()
