"""The host side of sketch representative selection (csrc/reps_resolve.hpp:
the in-block order from the cover flags, the block's tile and t, and pass 2's
self-mapping) is pure host code: a stand-alone program with its own main,
compiled with the host compiler under AddressSanitizer + UBSan, checks it
against a brute-force loop without a device (block sizes 1, 2 and ragged,
every row covered, no row covered, ties at t, NaN and 1.0 distances, two tie
ranks)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_reps_resolve_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "reps_resolve_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "reps_resolve_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
