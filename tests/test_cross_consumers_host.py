"""CPU: the fixture of the cross within / group_stats / histogram tests
(cross_consumers_ref.py) holds every condition those tests rely on; the three
entry points are declared, exported and bound, and refuse a null context
before any device work; and the expected answers the GPU tests compare with
agree with brute force on the sliced D."""
import ctypes as C
import os
import re

import numpy as np

import cross_consumers_ref as Z
import hist_ref as H
import within_ref as W

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ARITY = {"gdist_cross_within": 14, "gdist_cross_group_stats": 13, "gdist_cross_histogram": 16}


def test_fixture_conditions():
    Z.check_fixture()


def test_declared_exported_and_bound():
    from gdist import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdist.h")).read(), flags=re.S)
    dll = C.CDLL(_lib.LIB_PATH)
    for name, nargs in ARITY.items():
        m = re.search(r"\bint\s+" + name + r"\s*\(([^;]*?)\)\s*;", header)
        assert m, f"include/gdist.h does not declare {name}"
        assert len(m.group(1).split(",")) == nargs, name
        assert hasattr(dll, name), name
        assert name in _lib.EXPORTED
        assert len(getattr(_lib.lib, name).argtypes) == nargs


def test_null_context_is_einval():
    from gdist import _lib as L
    rowptr, cols, d = np.full(3, -7, np.int64), np.full(4, -7, np.int64), np.full(4, 7.5)
    total = C.c_int64(-7)
    L.lib.gdist_triangle_partition(-1, 4, 1, L.ptr(np.zeros(5, np.int64), C.c_int64))   # another message first
    rc = L.lib.gdist_cross_within(None, None, None, 0, 2, 0, 2, 0, 0.9, 4, L.ptr(rowptr, C.c_int64),
                                  L.ptr(cols, C.c_int64), L.ptr(d, C.c_double), C.byref(total))
    assert rc == L.EINVAL and b"null context" in L.lib.gdist_last_error()
    assert np.all(rowptr == -7) and np.all(cols == -7) and np.all(d == 7.5) and total.value == -7
    lab = np.zeros(4, np.int32)
    sides = np.full(2 * C.sizeof(L.GroupSide), 0x5A, np.uint8)
    bad = np.full(1, -7, np.int64)
    L.lib.gdist_triangle_partition(-1, 4, 1, L.ptr(np.zeros(5, np.int64), C.c_int64))
    rc = L.lib.gdist_cross_group_stats(None, None, None, 0, 2, 0, 2, 0, 1, L.ptr(lab, C.c_int32),
                                       L.ptr(lab, C.c_int32), sides.ctypes.data, L.ptr(bad, C.c_int64))
    assert rc == L.EINVAL and b"null context" in L.lib.gdist_last_error()
    assert np.all(sides == 0x5A) and bad[0] == -7
    edges = np.array([0.5])
    counts, nans = np.full(2, -7, np.int64), np.full(1, -7, np.int64)
    L.lib.gdist_triangle_partition(-1, 4, 1, L.ptr(np.zeros(5, np.int64), C.c_int64))
    rc = L.lib.gdist_cross_histogram(None, None, None, 0, 2, 0, 2, 0, 1, L.ptr(edges, C.c_double), 0, None, None,
                                     L.ptr(counts, C.c_int64), L.ptr(nans, C.c_int64), None)
    assert rc == L.EINVAL and b"null context" in L.lib.gdist_last_error()
    assert np.all(counts == -7) and np.all(nans == -7)


def test_within_expected_vs_brute_force():
    for flags in (0, Z.EMPTY_NAN):
        D = Z.expected_d(flags)
        for md in (0.9, 0.0, 1.0, -1.0, float("inf")):
            for rows, cols in ((None, None), ((5, 37), (64, 143)), ((40, 52), (5, 130))):
                r0, r1 = rows or (0, Z.NQ)
                c0, c1 = cols or (0, Z.NS)
                got = W.as_lists(*Z.within_expected(md, flags, rows, cols))
                assert got == W.within_brute(D[r0:r1, c0:c1], md, r0, c0, upper=False, keep_self=True)
    # a query index equal to a subject index means nothing: cell (5, 5) is listed like any other
    rp, cols, d = Z.within_expected(1.0, 0, rows=(5, 6))
    assert cols.tolist() == list(range(Z.NS))


def test_hist_expected_vs_brute_force():
    D = Z.expected_d(Z.EMPTY_NAN)
    for edges in (Z.EDGES50, Z.ulp_edges()):
        for rows, cols in ((None, None), ((5, 37), (64, 143))):
            r0, r1 = rows or (0, Z.NQ)
            c0, c1 = cols or (0, Z.NS)
            for labelled in (True, False):
                got = Z.hist_expected(edges, Z.EMPTY_NAN, rows, cols, labelled)
                want = H.hist_brute(D[r0:r1, c0:c1], edges, Z.LABELS if labelled else None, Z.NS + r0, c0,
                                    upper=False)
                for g, w in zip(got, want):
                    assert np.array_equal(g, w)


def test_series_totals_match_the_group_sides():
    """sum(counts) + nans of every series = n + ones + nans of its group side."""
    for flags in (0, Z.EMPTY_NAN):
        counts, nans, bad = Z.hist_expected(Z.EDGES50, flags)
        ref = Z.group_expected(flags)
        for t, r in enumerate(ref):
            assert bad[t] == r["bad"]
            for k, s in enumerate(r["sides"]):
                assert counts[2 * t + k].sum() + nans[2 * t + k] == s["n"] + s["ones"] + s["nans"]
            assert r["bad"] + sum(s["n"] + s["ones"] + s["nans"] for s in r["sides"]) == Z.NQ * Z.NS
