"""The wave-per-pair segmented merge of two sketch signatures
(csrc/sketch_cross_merge.hpp) is host and device code over plain pointers: a
stand-alone program with its own main, compiled with the host compiler under
AddressSanitizer + UBSan, runs the 64 lanes of a pair in a loop and compares
(common, taken) with a plain two-pointer merge, without a device (random pairs
of widths 1 .. 1000 and lengths 0 .. width on either side, identical, disjoint
and interleaved signatures, the cap at every position of a union, INT_MIN and
INT_MAX as hashes, na < 64 < nb)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_sketch_cross_merge_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "sketch_cross_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sketch_cross_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
