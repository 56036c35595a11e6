"""CPU: the distance-histogram entry point (gdist_histogram) is declared,
exported and bound; it refuses a null context without touching the device or
its outputs; the tests' reference answer (hist_ref) agrees with a brute-force
restatement; and the recipe fixture has the properties test_gpu_hist.py
relies on."""
import ctypes as C
import os
import re

import numpy as np

import closest_ref as R
import hist_ref as H

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
N = 195
EMPTY_NAN = 0x400
EDGES50 = np.array([i / 50 for i in range(51)])
MEDIAN = 0.9514426460239268


def make_labels(n):
    i = np.arange(n)
    return np.stack([i // 15, np.zeros(n, dtype=np.int64), i, np.where(i % 7 == 0, -1, i % 3)]).astype(np.int32)


def test_histogram_is_declared_exported_and_bound():
    from gdist import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdist.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gdist_histogram\s*\(([^;]*?)\)\s*;", header)
    assert m, "include/gdist.h does not declare gdist_histogram"
    assert len(m.group(1).split(",")) == 15
    t = re.search(r"\bint\s+gdist_ctx_histogram_timing\s*\(([^;]*?)\)\s*;", header)
    assert t and len(t.group(1).split(",")) == 3
    assert re.search(r"#define\s+GDIST_HIST_MAX_EDGES\s+1023\b", header) and _lib.HIST_MAX_EDGES == 1023
    dll = C.CDLL(_lib.LIB_PATH)
    for name in ("gdist_histogram", "gdist_ctx_histogram_timing"):
        assert hasattr(dll, name)
        assert name in _lib.EXPORTED
    assert _lib.lib.gdist_abi_version() == 1


def test_histogram_null_context_is_einval():
    from gdist import _lib
    counts, nans, bad = np.full(4, -7, np.int64), np.full(1, -7, np.int64), np.full(1, -7, np.int64)
    edges = np.array([0.25, 0.5, 1.0])
    _lib.lib.gdist_triangle_partition(-1, 4, 1, _lib.ptr(np.zeros(5, np.int64), C.c_int64))   # another message first
    rc = _lib.lib.gdist_histogram(None, None, 0, 2, 0, 2, _lib.METHOD_AUTO, 0, 3, _lib.ptr(edges, C.c_double), 0, None,
                                  _lib.ptr(counts, C.c_int64), _lib.ptr(nans, C.c_int64), _lib.ptr(bad, C.c_int64))
    assert rc == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error()
    assert np.all(counts == -7) and np.all(nans == -7) and np.all(bad == -7)
    m, s = C.c_double(7.5), C.c_double(7.5)
    assert _lib.lib.gdist_ctx_histogram_timing(None, C.byref(m), C.byref(s)) == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error() and (m.value, s.value) == (7.5, 7.5)


def test_histogram_class():
    import gdist
    e = np.array([0.5, 1.0])
    a = gdist.Histogram(e, [[1, 2, 3], [0, 0, 4]], [1, 0], [5])
    b = gdist.Histogram(e, [[10, 0, 0], [0, 7, 0]], [0, 2], [1])
    c = a + b
    assert c.counts.tolist() == [[11, 2, 3], [0, 7, 4]] and c.nans.tolist() == [1, 2] and c.bad.tolist() == [6]
    assert c.counts.dtype == np.int64 and c.edges.dtype == np.float64
    assert c.total.tolist() == [17, 13] and a.total.tolist() == [7, 4]
    assert c.tobytes() == (b + a).tobytes() != a.tobytes()
    assert len(c.tobytes()) == 8 * (6 + 2 + 1)
    for other in (gdist.Histogram(np.array([0.5, 0.75]), b.counts, b.nans, b.bad),       # other edges
                  gdist.Histogram(np.array([-0.0, 1.0]), b.counts, b.nans, b.bad),
                  gdist.Histogram(e, b.counts[:1], b.nans[:1], np.zeros(0, np.int64))):    # another shape
        try:
            a + other
        except ValueError:
            continue
        raise AssertionError("a sum of unlike histograms")
    assert (gdist.Histogram(np.array([0.0]), [[0, 1]], [0], []) + gdist.Histogram(np.array([0.0]), [[0, 2]], [0], [])
            ).counts.tolist() == [[0, 3]]


def test_hist_ref_vs_brute_force_small():
    """Random small matrices holding NaN, 0.0, 1.0 and values equal to edges."""
    rng = np.random.default_rng(5)
    nan = float("nan")
    tiny = 5e-324
    edge_sets = [np.array([0.0]), np.array([1.0]), np.array([0.25, 0.5, np.nextafter(0.5, 1.0), 1.0]),
                 np.array([-np.inf, 0.0, tiny, 1e-310, 0.5, np.inf]), np.array([-1.0, 2.0])]
    pool = np.array([nan, 0.0, 1.0, 0.25, 0.5, np.nextafter(0.5, 0.0), np.nextafter(0.5, 1.0), tiny, 1e-310, 0.75])
    for trial in range(6):
        n = 9 + trial
        D = pool[rng.integers(0, len(pool), size=(n, n))]
        lab = np.stack([rng.integers(-1, 3, size=n), np.zeros(n, dtype=np.int64)])
        for edges in edge_sets:
            for labels in (None, lab, lab[0]):
                for upper in (True, False):
                    for (r0, r1), (c0, c1) in (((0, n), (0, n)), ((2, 7), (1, n)), ((5, n), (0, 4))):
                        got = H.hist_ref(D[r0:r1, c0:c1], edges, labels, r0, c0, upper)
                        exp = H.hist_brute(D[r0:r1, c0:c1], edges, labels, r0, c0, upper)
                        for g, x in zip(got, exp):
                            assert g.dtype == np.int64 and g.shape == x.shape and np.array_equal(g, x), \
                                (trial, edges, upper, r0, r1, c0, c1)
    # by hand: a value on an edge belongs to the bucket above it
    counts, nans, bad = H.hist_ref(np.array([[0.0, 0.25, 0.5, 1.0, nan, 0.3]]), [0.25, 0.5, 1.0], upper=False)
    assert counts.tolist() == [[1, 2, 1, 1]] and nans.tolist() == [1] and bad.tolist() == []
    counts, nans, bad = H.hist_ref(np.array([[0.0, 0.5], [0.5, nan]]), [0.5], [0, -1], upper=False)
    assert counts.tolist() == [[1, 0], [0, 0]] and nans.tolist() == [0, 0] and bad.tolist() == [3]


def test_hist_ref_vs_brute_force_recipe():
    D = R.recipe()[3]
    lab = make_labels(N)
    for labels, upper in ((lab, True), (None, False)):
        got, exp = H.hist_ref(D, EDGES50, labels, upper=upper), H.hist_brute(D, EDGES50, labels, upper=upper)
        assert all(np.array_equal(g, x) for g, x in zip(got, exp))


def test_pattern_edges_and_rank():
    e = H.pattern_edges(1023)
    assert len(e) == 1023 and np.all(np.diff(e) > 0) and 0.0 < e[0] and e[-1] < 1.0
    assert np.all(np.diff(e.view(np.uint64).astype(np.int64)) >= (0x3FF0000000000000 // 1024) - 1)
    assert [H.rank_of(q, 18915) for q in (0, 0.01, 0.5, 1)] == [1, 190, 9458, 18915]
    assert H.rank_of(0.5, 1) == 1 and H.rank_of(1e-9, 10) == 1


def test_fixture_facts():
    """What test_gpu_hist.py relies on, on the oracle's matrix of the recipe."""
    D = R.recipe()[3]
    assert D.shape == (N, N)
    up = D[np.triu_indices(N, 1)]
    assert len(up) == 18915 and int((up == 1.0).sum()) == 7287 and int((up == 0.0).sum()) == 4
    assert len(np.unique(up)) == 1824 and not np.isnan(D).any()
    assert D.size == 38025 and int((D == 0.0).sum()) == 201 and int((D == 1.0).sum()) == 14576
    assert not np.signbit(D).any() and D.min() == 0.0 and D.max() == 1.0
    Dn = R.recipe(EMPTY_NAN)[3]
    assert int(np.isnan(Dn[np.triu_indices(N, 1)]).sum()) == 1 and int(np.isnan(Dn).sum()) == 4
    s = np.sort(up)
    assert s[H.rank_of(0.5, len(s)) - 1] == MEDIAN and int((up == MEDIAN).sum()) == 28
    counts, nans, bad = H.hist_ref(D, EDGES50)
    assert counts.shape == (1, 52) and nans.tolist() == [0] and bad.tolist() == []
    assert counts[0, -5:].tolist() == [1642, 1890, 1289, 98, 7287] and counts[0, 0] == 0
    assert int(counts.sum()) == 18915
    # the concentrated case: the ones and their 98 + 1289 neighbours in adjacent buckets
    assert H.hist_ref(D, [0.96, 0.98, 1.0])[0][0].tolist() == [18915 - 7287 - 98 - 1289, 1289, 98, 7287]
    # 1023 evenly spaced patterns: nearly all of them lie below every d > 0, the last near 0.5
    e = H.pattern_edges(1023)
    c = H.hist_ref(D, e)[0][0]
    assert c[0] == 4 and 0.5 < e[-1] < 0.51 and int(c.sum()) == 18915 and int((c > 0).sum()) >= 3
