"""Host side of the sketch-error sweep (gdist_width_sweep), without a device.

The lane-level arithmetic (csrc/width_sweep.hpp) is host and device code over
plain pointers: a stand-alone program with its own main, compiled with the
host compiler under AddressSanitizer + UBSan, runs the 64 lanes of a pair in a
loop and compares the per-size (common, taken) and distance with a plain
two-pointer merge of the two prefixes at every size (random pairs of widths
1 .. 1000 and lengths 0 .. width on either side, identical, disjoint and
interleaved signatures, INT_MIN and INT_MAX as hashes, na < 64 < nb, size
lists of 1, 64, 65 and 130 entries, sizes 1 and = width, sizes above both
lengths, signatures wider than the last size, both modes).

The expected answers the GPU tests use (width_sweep_ref: prefix signatures of
one build at the largest size, exact integer sums) agree with the flat loop of
test_gpu_parity.test_width_processor_vs_restatement (pyref sets, one sketch
build a size, doubles added in i-major order)."""
import os
import shutil
import subprocess

import pytest

import pyref
import width_sweep_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_width_sweep_lanes_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "width_sweep_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "width_sweep_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def scene_groups():
    """The groups of the width test's scene: 14 and 11 proteins, at most 12 a group."""
    from gdist import synth
    g1 = [bytes(r) for r in synth.genomes(14, 300, 0.10, 107, protein=True)]
    g2 = [bytes(r) for r in synth.genomes(11, 250, 0.30, 108, protein=True)]
    return [g1[:12], g1[12:], g2]


@pytest.mark.parametrize("flags", [0, pyref.SKETCH_JACCARD])
def test_reference_agrees_with_the_flat_loop(flags):
    sizes = (20, 40, 60)
    for prots in scene_groups():
        n = len(prots)
        pairs, rows = R.expected(prots, 8, pyref.PROT, sizes, flags)
        sets = [pyref.kmer_set(p.decode(), 8, pyref.PROT) for p in prots]
        real = {(i, j): pyref.set_distance(sets[i], sets[j]) for i in range(n) for j in range(i + 1, n)}
        assert pairs == sum(1 for v in real.values() if v < 1.0)
        for size, row in zip(sizes, rows):
            sk = [pyref.sketch(s, size) for s in sets]
            differing, total, mx = 0, 0.0, 0.0
            for i in range(n):
                for j in range(i + 1, n):
                    sd = pyref.sketch_distance(sk[i], sk[j], size, flags)[0]
                    r = real[(i, j)]
                    if r != sd:
                        e = abs(r - sd) * 2.0 / (r + sd)
                        differing += 1
                        mx = e if e > mx else mx
                        total += e
            assert row["size"] == size and row["dwarves"] == sum(1 for x in sk if len(x) < size)
            assert row["differing"] == differing and row["max_err"] == mx
            # the flat sum rounds once a term (fewer than n^2 / 2 of them), each time by at most 2^-53 of
            # the running total; the exact sum quantises each term by at most 2^-63 and rounds once
            assert abs(row["total"] - total) <= n * n * 2.0 ** -52 * total
            assert row["total"] == float(row["sum"]) * 2.0 ** -62 and row["mean"] == row["total"] / pairs
