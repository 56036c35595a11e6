"""The unit plan of the cross-collection join (csrc/cross_plan.hpp) is pure
host code: a stand-alone program with its own main, compiled with the host
compiler under AddressSanitizer + UBSan, checks it without a device (every
(non-empty row, column block, segment) covered by exactly one unit; the cut
count clamped to [1, nseg]; nseg = 1, a ragged last block, empty rows, one
row, zero columns; the budget at both clamps; the column-block-major order;
every unit walked by exactly one workgroup)."""
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_cross_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "cross_plan_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cross_plan_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
