"""CPU: the pair-list entry point (gdist_pairs) is declared, exported and
bound; it refuses a null context without touching its outputs; and the tests'
reference answer (pairs_ref: fancy indexing of the oracle's matrices) equals a
pair-by-pair loop over oracle.intersect / oracle.distance."""
import ctypes as C
import os
import re

import numpy as np

import closest_ref as CR
import pairs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_pairs_is_declared_exported_and_bound():
    from gdist import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdist.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gdist_pairs\s*\(([^;]*?)\)\s*;", header)
    assert m, "include/gdist.h does not declare gdist_pairs"
    assert len(m.group(1).split(",")) == 9
    t = re.search(r"\bint\s+gdist_ctx_pairs_info\s*\(([^;]*?)\)\s*;", header)
    assert t and len(t.group(1).split(",")) == 4
    dll = C.CDLL(_lib.LIB_PATH)
    for name in ("gdist_pairs", "gdist_ctx_pairs_info"):
        assert hasattr(dll, name)
        assert name in _lib.EXPORTED
    assert _lib.lib.gdist_abi_version() == 1


def test_pairs_null_context_is_einval():
    from gdist import _lib
    rows, cols = np.zeros(3, np.int64), np.zeros(3, np.int64)
    I, D = np.full(3, -7, np.int32), np.full(3, 7.5)
    _lib.lib.gdist_triangle_partition(-1, 4, 1, _lib.ptr(np.zeros(5, np.int64), C.c_int64))   # another message first
    rc = _lib.lib.gdist_pairs(None, None, 3, _lib.ptr(rows, C.c_int64), _lib.ptr(cols, C.c_int64), _lib.METHOD_AUTO,
                              0, _lib.ptr(I, C.c_int32), _lib.ptr(D, C.c_double))
    assert rc == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error()
    assert np.all(I == -7) and np.all(D == 7.5)
    ms, g, u = C.c_double(7.5), C.c_int64(-7), C.c_int64(-7)
    assert _lib.lib.gdist_ctx_pairs_info(None, C.byref(ms), C.byref(g), C.byref(u)) == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error() and (ms.value, g.value, u.value) == (7.5, -7, -7)


def test_pairs_ref_vs_brute_force():
    _, off, codes, _ = CR.recipe()
    lists = R.recipe_lists()
    assert sorted(lists) == ["long_group", "mixed", "singletons", "unit_edges"]
    for flags in (0, 0x400):
        I, D = R.recipe_matrices(flags)
        for name in ("singletons", "unit_edges"):
            rows, cols = lists[name]
            gI, gD = R.pairs_ref(I, D, rows, cols)
            bI, bD = R.pairs_brute(off, codes, rows, cols, flags)
            assert gI.dtype == np.int32 and gD.dtype == np.float64 and len(gI) == len(gD) == len(rows)
            assert np.array_equal(gI, bI)
            assert np.array_equal(gD.view(np.uint64), bD.view(np.uint64))
        # the self pairs and the empty sets, which the matrix's diagonal fill decides
        rows = np.array([R.NONEMPTY, R.EMPTY_A, R.EMPTY_A, R.EMPTY_B, 5], np.int64)
        cols = np.array([R.NONEMPTY, R.EMPTY_A, R.EMPTY_B, R.EMPTY_B, 151], np.int64)
        gI, gD = R.pairs_ref(I, D, rows, cols)
        bI, bD = R.pairs_brute(off, codes, rows, cols, flags)
        assert np.array_equal(gI, bI) and np.array_equal(gD.view(np.uint64), bD.view(np.uint64))
        assert gI[0] == off[R.NONEMPTY + 1] - off[R.NONEMPTY] > 0 and gD[0] == 0.0
        assert gI[1:4].tolist() == [0, 0, 0]
        assert np.isnan(gD[1:4]).all() if flags else (gD[1:4] == 1.0).all()


def test_recipe_lists_have_the_shapes_the_gpu_tests_rely_on():
    lists = R.recipe_lists()
    rows, cols = lists["singletons"]
    assert len(rows) == R.N and len(np.unique(rows)) == R.N
    rows, cols = lists["long_group"]
    assert sorted(cols[rows == R.NONEMPTY].tolist()) == list(range(R.N)) and len(np.unique(rows)) > 20
    rows, cols = lists["unit_edges"]
    assert sorted(np.unique(rows, return_counts=True)[1].tolist()) == [1, 63, 64, 65, 128, 129]
    rows, cols = lists["mixed"]
    pairs = list(zip(rows.tolist(), cols.tolist()))
    assert len(pairs) == 2000 and len(set(pairs)) < 2000
    for p in ((R.NONEMPTY, R.NONEMPTY), (R.EMPTY_A, R.EMPTY_A), (R.EMPTY_A, R.EMPTY_B)):
        assert p in pairs
    assert pairs.count((12, 90)) >= 2
