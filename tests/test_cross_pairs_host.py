"""CPU: what the cross pair-list tests (gdist_cross_pairs) rely on holds
without a device. The fixtures' properties are asserted from the oracle's side
(cross_pairs_ref.check_fixture); the reference answer equals a pair-by-pair
loop over the oracle; the entry point is declared, exported and bound and
refuses a null context without touching its outputs; and the cut-point search
of the join kernel (csrc/cross_cut.hpp) is pure host-and-device code that a
stand-alone program with its own main, compiled with the host compiler under
AddressSanitizer + UBSan, runs over rows that are empty, below every splitter,
above every splitter, inside one segment and on the splitters, nseg 1 .. 4,096."""
import ctypes as C
import os
import re
import shutil
import subprocess

import numpy as np
import pytest

import cross_pairs_ref as P
import cross_ref as X
import pairs_ref

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_has_the_shapes_the_gpu_tests_rely_on():
    P.check_fixture()


def test_ref_vs_brute_force():
    """The expected cells equal pairs_brute on the oracle's pack of subjects +
    queries for the pair (NS + row, col), the contract's concat form."""
    off, codes = X.packed()
    L = P.lists()
    for flags in (0, P.EMPTY_NAN):
        for name in ("singletons", "unit_edges"):
            rows, cols = L[name]
            gI, gD = P.pairs_ref(flags, rows, cols)
            bI, bD = pairs_ref.pairs_brute(off, codes, rows + P.NS, cols, flags)
            assert gI.dtype == np.int32 and gD.dtype == np.float64 and len(gI) == len(gD) == len(rows)
            assert np.array_equal(gI, bI)
            assert np.array_equal(gD.view(np.uint64), bD.view(np.uint64))


def test_cross_pairs_is_declared_exported_and_bound():
    from gdist import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdist.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gdist_cross_pairs\s*\(([^;]*?)\)\s*;", header)
    assert m, "include/gdist.h does not declare gdist_cross_pairs"
    assert len(m.group(1).split(",")) == 9
    assert hasattr(C.CDLL(_lib.LIB_PATH), "gdist_cross_pairs") and "gdist_cross_pairs" in _lib.EXPORTED


def test_cross_pairs_null_context_is_einval():
    from gdist import _lib
    rows, cols = np.zeros(3, np.int64), np.zeros(3, np.int64)
    I, D = np.full(3, -7, np.int32), np.full(3, 7.5)
    rc = _lib.lib.gdist_cross_pairs(None, None, None, 3, _lib.ptr(rows, C.c_int64), _lib.ptr(cols, C.c_int64), 0,
                                    _lib.ptr(I, C.c_int32), _lib.ptr(D, C.c_double))
    assert rc == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error()
    assert np.all(I == -7) and np.all(D == 7.5)


def test_cut_points_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "cross_cut_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "cross_cut_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
