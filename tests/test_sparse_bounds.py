"""The sparse plan's chunk bounds at equal modelled cost (csrc/sparse_bounds.hpp)
are pure host code: a stand-alone program with its own main, compiled with
the host compiler under AddressSanitizer + UBSan, checks them without a
device (flat costs, a 20 x heavier tail, one huge granule; counts 1, 2, 7, 62
and more than the granules; fold slabs 0, 2 and the count; a predicate that
refuses every range longer than the cap)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_balanced_bounds_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "sparse_bounds_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sparse_bounds_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
