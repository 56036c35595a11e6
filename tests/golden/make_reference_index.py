"""Generates tests/golden/reference_index.json, what tests/test_citations.py
knows of the reference sources (which are not part of this repository): the
line count of every reference file, and one hash for every (reference file,
cited lines, literal) in the host code whose literal stands on the lines
cited for it. Refuses to write when a cited literal is not on its lines.
Run: python tests/golden/make_reference_index.py REFERENCE_JAVA_SOURCE_DIR
"""
import glob
import json
import os
import sys

HERE = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.dirname(HERE))

import test_citations as tc  # noqa: E402


def main(ref_dir):
    ref = {}
    for p in sorted(glob.glob(os.path.join(ref_dir, "**", "*.java"), recursive=True)):
        with open(p, errors="replace") as f:
            ref[os.path.basename(p)] = f.read().split("\n")
    if not ref:
        sys.exit(f"no reference sources under {ref_dir}")
    keys, bad = set(), []
    for path, ln, name, ranges, lit, probe in tc._cited_literals():
        if name not in ref:
            continue
        text = "\n".join("\n".join(ref[name][a - 1:b]) for a, b in ranges)
        if probe in text:
            keys.add(tc.literal_key(name, ranges, probe))
        else:
            bad.append(f"{os.path.relpath(path, tc.ROOT)}:{ln}: {lit!r} not on {name}:{ranges}")
    if bad:
        sys.exit("\n".join(bad))
    with open(tc.INDEX, "w") as f:
        json.dump({"lines": {k: len(v) for k, v in sorted(ref.items())},
                   "literals_on_cited_lines": sorted(keys)}, f, indent=1)
        f.write("\n")
    print(f"{len(ref)} reference files, {len(keys)} cited literals -> {os.path.relpath(tc.INDEX, tc.ROOT)}")


if __name__ == "__main__":
    if len(sys.argv) != 2:
        sys.exit(__doc__)
    main(sys.argv[1])
