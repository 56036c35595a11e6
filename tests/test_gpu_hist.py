"""Distribution of the distances over bucket edges on the device
(gdist_histogram), the exact order statistics built on it (quantiles) and the
--dist table (processors.distance_distribution), over a device-resident
collection. Every count is compared with `==` against hist_ref on the oracle's
distance matrix. Outputs are pre-filled with garbage, so a field the call
leaves unwritten fails. The properties of the fixture the tests rely on are
asserted on the oracle's matrix in test_hist_host.py."""
import ctypes as C
import functools
import io

import numpy as np
import pytest

import closest_ref as R
import hist_ref as H

pytestmark = pytest.mark.gpu

N = 195
EMPTY_NAN, SKETCH_JACCARD, UPPER_TRIANGLE, OUT_DEVICE = 0x400, 0x800, 0x100, 0x200
TYPES = ("block", "one", "solo", "holes")
EDGES50 = np.array([i / 50 for i in range(51)])
MEDIAN = 0.9514426460239268
GARBAGE = -9


def make_labels(n):
    i = np.arange(n)
    return np.stack([i // 15, np.zeros(n, dtype=np.int64), i, np.where(i % 7 == 0, -1, i % 3)]).astype(np.int32)


LABELS = make_labels(N)


def raw_hist(sets, edges, labels=None, rows=None, cols=None, upper=True, method=0, flags=0):
    """gdist_histogram into garbage-filled outputs: (rc, counts [S, E + 1], nans [S], bad [T])."""
    from gdist import _lib as L
    edges = np.ascontiguousarray(edges, dtype=np.float64)
    T = 0 if labels is None else np.atleast_2d(labels).shape[0]
    lab = None if labels is None else np.ascontiguousarray(np.atleast_2d(labels), dtype=np.int32)
    ns = len(sets)
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    S = 2 * T if T else 1
    counts = np.full((S, len(edges) + 1), GARBAGE, dtype=np.int64)
    nans, bad = np.full(S, GARBAGE, dtype=np.int64), np.full(T, GARBAGE, dtype=np.int64)
    fl = flags | (UPPER_TRIANGLE if upper else 0)
    rc = L.lib.gdist_histogram(sets.ctx.h, sets.h, r0, r1, c0, c1, method, fl, len(edges), L.ptr(edges, C.c_double),
                               T, L.ptr(lab, C.c_int32) if T else None, L.ptr(counts, C.c_int64),
                               L.ptr(nans, C.c_int64), L.ptr(bad, C.c_int64) if T else None)
    return rc, counts, nans, bad


def raw_bytes(*a, **kw):
    rc, counts, nans, bad = raw_hist(*a, **kw)
    assert rc == 0
    return counts.tobytes() + nans.tobytes() + bad.tobytes()


def check(sets, D, edges, labels=None, rows=None, cols=None, upper=True, method=0, flags=0):
    """The call against hist_ref on D (the whole collection's matrix); returns the bytes."""
    ns = D.shape[0]
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    rc, counts, nans, bad = raw_hist(sets, edges, labels, rows, cols, upper, method, flags)
    assert rc == 0
    ec, en, eb = H.hist_ref(D[r0:r1, c0:c1], edges, labels, r0, c0, upper)
    where = f"rows {rows} cols {cols} upper {upper} method {method}"
    assert np.array_equal(counts, ec), where
    assert np.array_equal(nans, en) and np.array_equal(bad, eb), where
    return counts.tobytes() + nans.tobytes() + bad.tobytes()


@functools.lru_cache(maxsize=None)
def sorted_d(upper):
    """The non-NaN distances of the recipe's triangle / full square, ascending."""
    D = R.recipe()[3]
    return np.sort(D[np.triu_indices(N, 1)] if upper else D.ravel())


@pytest.fixture(scope="module")
def kset(ctx):
    import gdist
    seqs, _, _, D = R.recipe()
    assert D.shape == (N, N)
    s = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "full"])
@pytest.mark.parametrize("method", [1, 2, 0], ids=["sorted", "bitset", "auto"])
def test_methods_and_regions(kset, method, upper):
    D = R.recipe()[3]
    for labels in (None, LABELS):
        got = check(kset, D, EDGES50, labels, upper=upper, method=method)
        assert raw_bytes(kset, EDGES50, labels, upper=upper, method=method) == got   # a second call: identical bytes
        assert raw_bytes(kset, EDGES50, labels, upper=upper, method=1) == got        # and whatever the method
    rc, counts, nans, bad = raw_hist(kset, EDGES50, upper=upper, method=method)
    if upper:
        assert counts[0, -5:].tolist() == [1642, 1890, 1289, 98, 7287] and counts[0, 0] == 0
    assert int(counts.sum()) == (18915 if upper else 38025) and nans.tolist() == [0] and len(bad) == 0


@pytest.mark.parametrize("rows_,cols_", [(7, 33), (64, 100), (128, 193), (1, 64)])
def test_block_sizes(kset, opts, rows_, cols_):
    """Several row blocks and column chunks, ragged last ones, chunks left of,
    on and right of the diagonal, one row a block: identical bytes."""
    assert N % cols_ != 0 and N > cols_
    want = {(u, t): raw_bytes(kset, EDGES50, lab, upper=u)
            for u in (True, False) for t, lab in enumerate((None, LABELS))}
    opts(closest_rows=rows_, closest_cols=cols_)
    for (u, t), w in want.items():
        for method in ((1, 2) if rows_ > 1 else (0,)):     # one row a block: 780 steps a call
            assert raw_bytes(kset, EDGES50, (None, LABELS)[t], upper=u, method=method) == w


def test_rectangles(kset):
    D = R.recipe()[3]
    for method in (1, 2):
        for labels in (None, LABELS):
            for upper in (True, False):
                check(kset, D, EDGES50, labels, rows=(3, 77), cols=(50, 160), upper=upper, method=method)
            check(kset, D, EDGES50, labels, rows=(150, 195), cols=(0, 150), upper=False, method=method)
    # wholly left of the diagonal with upper: no pair
    for labels in (None, LABELS):
        got = check(kset, D, EDGES50, labels, rows=(100, 195), cols=(0, 100), upper=True)
        assert not any(got)
        # empty ranges answer the same, GDIST_OK and every output zero
        assert raw_bytes(kset, EDGES50, labels, rows=(5, 5)) == got
        assert raw_bytes(kset, EDGES50, labels, rows=(5, 9), cols=(20, 20)) == got
    # two disjoint row ranges add to the whole
    for upper in (True, False):
        whole = kset.histogram(EDGES50, LABELS, upper=upper)
        a = kset.histogram(EDGES50, LABELS, rows=(0, 100), upper=upper)
        b = kset.histogram(EDGES50, LABELS, rows=(100, N), upper=upper)
        assert whole.tobytes() == raw_bytes(kset, EDGES50, LABELS, upper=upper)
        assert (a + b).tobytes() == whole.tobytes() == (b + a).tobytes() and a.tobytes() != whole.tobytes()
        assert whole.counts.shape == (8, 52) and whole.nans.shape == (8,) and whole.bad.shape == (4,)
    with pytest.raises(ValueError):
        a + kset.histogram(EDGES50[:-1], LABELS, rows=(100, N))
    with pytest.raises(ValueError):
        a + kset.histogram(EDGES50, rows=(100, N))


def test_edge_exactness(kset):
    D = R.recipe()[3]
    inf = float("inf")
    # one ulp either side of the median: the 28 pairs holding it, and no other, in [m, next)
    e = np.array([np.nextafter(MEDIAN, 0.0), MEDIAN, np.nextafter(MEDIAN, 2.0)])
    for method in (1, 2):
        check(kset, D, e, method=method)
        check(kset, D, e, LABELS, upper=False, method=method)
    rc, counts, nans, _ = raw_hist(kset, e)
    assert rc == 0 and counts[0, 2] == 28 and counts[0, 1] == 0 and counts[0, 0] < 9458 <= counts[0, 0] + 28
    # a single edge at 1.0 separates the ones; one at 0.0 has nothing below it
    rc, counts, nans, _ = raw_hist(kset, [1.0])
    assert rc == 0 and counts.tolist() == [[18915 - 7287, 7287]] and nans.tolist() == [0]
    rc, counts, nans, _ = raw_hist(kset, [0.0])
    assert rc == 0 and counts.tolist() == [[0, 18915]] and nans.tolist() == [0]
    rc, counts, nans, _ = raw_hist(kset, [0.0], flags=EMPTY_NAN)
    assert rc == 0 and counts.tolist() == [[0, 18914]] and nans.tolist() == [1]
    # edges below every d, above every d, and the infinities
    for e, want in (([-1.0], [0, 18915]), ([-inf], [0, 18915]), ([2.0], [18915, 0]), ([inf], [18915, 0]),
                    ([-inf, inf], [0, 18915, 0]), ([-inf, -1.0, 0.0, 1.0, np.nextafter(1.0, 2.0), inf],
                                                   [0, 0, 0, 18915 - 7287, 7287, 0, 0])):
        rc, counts, nans, _ = raw_hist(kset, e)
        assert rc == 0 and counts.tolist() == [want] and nans.tolist() == [0], e
    # denormal edges: the 201 zeros of the full square below them, everything else above
    rc, counts, nans, _ = raw_hist(kset, [5e-324, 1e-310], upper=False)
    assert rc == 0 and counts.tolist() == [[201, 0, 38025 - 201]] and nans.tolist() == [0]
    check(kset, D, [5e-324, 1e-310], LABELS, upper=False)


def test_bucket_counts(kset):
    """The fewest and the most buckets, and the concentrated case: 8,674 of the
    18,915 pairs in three adjacent buckets."""
    D = R.recipe()[3]
    check(kset, D, [0.5])
    check(kset, D, [0.5], LABELS, upper=False)
    e = H.pattern_edges(1023)
    assert len(e) == 1023
    for method in (1, 2):
        check(kset, D, e, method=method)
        check(kset, D, e, LABELS, upper=False, method=method)
    # 1023 edges where the distances are: one ulp apart, up from the median
    m = int(np.float64(MEDIAN).view(np.uint64))
    near = (np.arange(1023, dtype=np.uint64) + np.uint64(m - 500)).view(np.float64)
    check(kset, D, near, LABELS)
    # ... and evenly spaced over [0.9, 1.0]
    check(kset, D, np.linspace(0.9, 1.0, 1023), LABELS, upper=False)
    rc, counts, nans, _ = raw_hist(kset, [0.96, 0.98, 1.0])
    assert rc == 0 and counts.tolist() == [[18915 - 7287 - 98 - 1289, 1289, 98, 7287]]
    check(kset, D, [0.96, 0.98, 1.0], LABELS, upper=False)


def test_two_segments(ctx):
    """4200 sets {0, i + 1}: a row is two work items (4096 + 104 columns) and
    the region two row blocks. Every pair shares one kmer of three, d = fl(1 -
    fl(1 / 3)) off the diagonal and 0.0 on it: one run a lane, expected
    counts in closed form."""
    import gdist
    n = 4200
    off = np.arange(n + 1, dtype=np.int64) * 2
    codes = np.stack([np.zeros(n, dtype=np.uint64), np.arange(1, n + 1, dtype=np.uint64)], axis=1).ravel()
    d = 1.0 - 1.0 / 3.0
    e = [0.0, np.nextafter(d, 0.0), d, np.nextafter(d, 1.0), 1.0]
    lab = np.stack([(np.arange(n) % 2), np.where(np.arange(n) == 4100, -1, 0)]).astype(np.int32)
    same = 2 * (n // 2) * (n // 2 - 1)                 # ordered off-diagonal pairs of equal parity
    s = gdist.KmerSets.from_codes(off, codes, 21, gdist.KmerType.DNA, ctx)
    for method in (1, 2):
        rc, counts, nans, _ = raw_hist(s, e, upper=False, method=method)
        assert rc == 0 and counts.tolist() == [[0, n, 0, n * (n - 1), 0, 0]] and nans.tolist() == [0]
        rc, counts, nans, _ = raw_hist(s, e, upper=True, method=method)
        assert rc == 0 and counts.tolist() == [[0, 0, 0, n * (n - 1) // 2, 0, 0]] and nans.tolist() == [0]
    rc, counts, nans, bad = raw_hist(s, e, lab, upper=False)
    assert rc == 0 and not nans.any() and bad.tolist() == [0, 2 * n - 1]
    assert counts.tolist() == [[0, n, 0, same, 0, 0], [0, 0, 0, n * n - n - same, 0, 0],
                               [0, n - 1, 0, (n - 1) * (n - 2), 0, 0], [0] * 6]
    s.free()


def test_against_group_stats(kset):
    """Series totals equal n + ones + nans of group_stats on the device, the
    bucket above an edge at 1.0 equals its ones, and bad is equal."""
    for upper in (True, False):
        for flags in (0, EMPTY_NAN):
            st = kset.group_stats(LABELS, upper=upper, flags=flags)
            h = kset.histogram(EDGES50, LABELS, upper=upper, flags=flags)
            assert h.total.tolist() == (st.n + st.ones + st.nans).ravel().tolist()
            assert h.counts[:, -1].tolist() == st.ones.ravel().tolist()
            assert h.nans.tolist() == st.nans.ravel().tolist() and h.bad.tolist() == st.bad.tolist()
            assert h.counts[:, 1:-1].sum(axis=1).tolist() == st.n.ravel().tolist() and not h.counts[:, 0].any()


def test_empty_nan(kset):
    D = R.recipe(EMPTY_NAN)[3]
    for method in (1, 2):
        for upper, n in ((True, 1), (False, 4)):
            rc, counts, nans, _ = raw_hist(kset, EDGES50, upper=upper, method=method, flags=EMPTY_NAN)
            assert rc == 0 and nans.tolist() == [n]
            assert int(counts.sum()) + n == (18915 if upper else 38025)
            check(kset, D, EDGES50, upper=upper, method=method, flags=EMPTY_NAN)
            check(kset, D, EDGES50, LABELS, upper=upper, method=method, flags=EMPTY_NAN)


@pytest.mark.parametrize("flags", [0, SKETCH_JACCARD], ids=["mash", "jaccard"])
def test_sketches(kset, opts, flags):
    sk = kset.sketches(64)
    _, D = sk.matrix(flags=flags)
    assert D.shape == (N, N) and len(np.unique(D[~np.isnan(D)])) > 3
    got = check(sk, D, EDGES50, flags=flags)
    assert raw_bytes(sk, EDGES50, flags=flags, method=77) == got                  # sketches ignore the method
    full = check(sk, D, EDGES50, LABELS, upper=False, flags=flags)
    check(sk, D, EDGES50, LABELS, rows=(100, 195), cols=(0, 120), upper=False, flags=flags)
    check(sk, D, H.pattern_edges(1023), flags=flags)
    h = sk.histogram(EDGES50, flags=flags)
    assert h.tobytes() == got
    s = np.sort(D[np.triu_indices(N, 1)])
    s = s[~np.isnan(s)]
    vals, n, calls = sk.quantiles([0.0, 0.5, 1.0], flags=flags)
    assert n == len(s) and calls <= 9
    assert vals.view(np.uint64).tolist() == s[[H.rank_of(q, n) - 1 for q in (0.0, 0.5, 1.0)]].view(np.uint64).tolist()
    opts(closest_rows=50, closest_cols=37)
    assert raw_bytes(sk, EDGES50, flags=flags) == got
    assert raw_bytes(sk, EDGES50, LABELS, upper=False, flags=flags) == full
    sk.free()


QS = (0.0, 0.01, 0.05, 0.25, 0.5, 0.75, 1.0)


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "full"])
def test_quantiles(kset, upper):
    """Order statistics bit for bit: np.sort of the oracle's D at rank k."""
    s = sorted_d(upper)
    want = np.array([s[H.rank_of(q, len(s)) - 1] for q in QS])
    vals, n, calls = kset.quantiles(QS, upper=upper)
    assert n == len(s) and calls <= 9 and vals.dtype == np.float64
    assert vals.view(np.uint64).tolist() == want.view(np.uint64).tolist()
    if upper:
        assert vals[4] == MEDIAN
    else:
        assert vals[0] == 0.0 and not np.signbit(vals[0])        # through the denormal edges
    assert vals[-1] == 1.0
    for q, w in zip(QS, want):
        v, n1, c1 = kset.quantiles(q, upper=upper)
        assert n1 == n and c1 <= 7 and v.shape == (1,)
        assert v.view(np.uint64)[0] == np.float64(w).view(np.uint64), q


def test_quantiles_edge_cases(kset):
    # NaN distances are not values; no value at all gives NaN
    s = sorted_d(False)
    vals, n, calls = kset.quantiles([0.5], upper=False, flags=EMPTY_NAN)
    D = R.recipe(EMPTY_NAN)[3].ravel()
    sn = np.sort(D[~np.isnan(D)])
    assert n == len(s) - 4 == len(sn) and vals[0] == sn[H.rank_of(0.5, n) - 1]
    vals, n, calls = kset.quantiles([0.0, 1.0], rows=(100, 195), cols=(0, 100))
    assert n == 0 and calls == 1 and np.isnan(vals).all() and vals.shape == (2,)
    # a rectangle, another method
    sub = np.sort(R.recipe()[3][3:77, 50:160].ravel())
    vals, n, calls = kset.quantiles([0.1, 0.9], rows=(3, 77), cols=(50, 160), upper=False, method=1)
    assert n == len(sub) and [float(v) for v in vals] == [sub[H.rank_of(q, n) - 1] for q in (0.1, 0.9)]
    for bad in ([-0.1], [1.5], [float("nan")], [0.1] * 9):
        with pytest.raises(ValueError):
            kset.quantiles(bad)
    vals, n, calls = kset.quantiles([])
    assert vals.shape == (0,) and calls == 0


def test_errors_leave_the_outputs_untouched(kset, ctx):
    import gdist
    from gdist import _lib as L
    nan, inf = float("nan"), float("inf")

    def einval(sets, edges, labels=LABELS, **kw):
        rc, counts, nans, bad = raw_hist(sets, edges, labels, **kw)
        assert rc == L.EINVAL and L.lib.gdist_last_error()
        assert np.all(counts == GARBAGE) and np.all(nans == GARBAGE) and np.all(bad == GARBAGE)

    for labels in (LABELS, None):
        einval(kset, EDGES50, labels, rows=(0, N + 1))
        einval(kset, EDGES50, labels, rows=(-1, 5))
        einval(kset, EDGES50, labels, rows=(9, 5))
        einval(kset, EDGES50, labels, cols=(0, N + 1))
        einval(kset, EDGES50, labels, cols=(7, 3))
        einval(kset, EDGES50, labels, flags=OUT_DEVICE)
        einval(kset, EDGES50, labels, method=3)
        einval(kset, EDGES50, labels, method=-1)
        einval(kset, [0.5, nan], labels)
        einval(kset, [nan], labels)
        einval(kset, [0.5, 0.5], labels)
        einval(kset, [0.5, 0.25], labels)
        einval(kset, [-0.0, 0.0], labels)
        einval(kset, [0.0, -0.0], labels)
        einval(kset, [inf, inf], labels)
        einval(kset, np.arange(1024, dtype=np.float64), labels)           # one edge too many
        einval(kset, EDGES50, labels, rows=(5, 5), method=3)                # decided before the empty range is
        einval(kset, [0.5, nan], labels, rows=(5, 5))
    # nedges 0 and negative, ntypes out of range, null pointers: straight through ctypes
    counts, nans, bad = (np.full(9 * 2 * 52, GARBAGE, dtype=np.int64), np.full(18, GARBAGE, dtype=np.int64),
                         np.full(9, GARBAGE, dtype=np.int64))
    lab9 = np.zeros((9, N), dtype=np.int32)
    ep, lp = L.ptr(EDGES50, C.c_double), L.ptr(lab9, C.c_int32)
    cp, np_, bp = L.ptr(counts, C.c_int64), L.ptr(nans, C.c_int64), L.ptr(bad, C.c_int64)
    args = (ctx.h, kset.h, 0, N, 0, N, 0, 0)
    for ne in (0, -1, 1024):
        assert L.lib.gdist_histogram(*args, ne, ep, 1, lp, cp, np_, bp) == L.EINVAL
    for T in (9, -1):
        assert L.lib.gdist_histogram(*args, 51, ep, T, lp, cp, np_, bp) == L.EINVAL
    assert L.lib.gdist_histogram(*args, 51, None, 1, lp, cp, np_, bp) == L.EINVAL
    assert L.lib.gdist_histogram(*args, 51, ep, 1, lp, None, np_, bp) == L.EINVAL
    assert L.lib.gdist_histogram(*args, 51, ep, 1, lp, cp, None, bp) == L.EINVAL
    assert L.lib.gdist_histogram(*args, 51, ep, 1, None, cp, np_, bp) == L.EINVAL
    assert L.lib.gdist_histogram(*args, 51, ep, 1, lp, cp, np_, None) == L.EINVAL
    assert L.lib.gdist_histogram(ctx.h, None, 0, 2, 0, 2, 0, 0, 51, ep, 1, lp, cp, np_, bp) == L.EINVAL
    assert np.all(counts == GARBAGE) and np.all(nans == GARBAGE) and np.all(bad == GARBAGE)
    # ntypes == 0 takes null labels and a null bad_out
    assert L.lib.gdist_histogram(*args, 51, ep, 0, None, cp, np_, None) == 0
    assert int(counts[:52].sum()) == 38025 and np.all(counts[52:] == GARBAGE) and nans[0] == 0 and nans[1] == GARBAGE
    with pytest.raises(ValueError):
        kset.histogram(EDGES50, LABELS[:, :10])
    with pytest.raises(ValueError):
        kset.histogram(EDGES50, lab9)
    with pytest.raises(ValueError):
        kset.histogram([])
    with pytest.raises(ValueError):
        kset.histogram([0.5, 0.25])
    # a bitsets-only collection: SORTED is refused, BITSET and AUTO answer
    b = gdist.KmerSets.from_sequences(R.recipe_sequences(), 21, gdist.KmerType.DNA, 0, ctx)
    b.build_bitsets()
    b.release_codes()
    einval(b, EDGES50, method=1)
    einval(b, EDGES50, None, method=1)
    want = raw_bytes(kset, EDGES50, LABELS)
    assert raw_bytes(b, EDGES50, LABELS, method=2) == want and raw_bytes(b, EDGES50, LABELS, method=0) == want
    b.free()


def test_timing_option(kset, ctx, opts):
    assert raw_bytes(kset, EDGES50, LABELS) and ctx.histogram_timing() == (-1.0, -1.0)
    opts(time_kernels=1)
    want = raw_bytes(kset, EDGES50, LABELS)
    matrix_ms, reduce_ms = ctx.histogram_timing()
    assert matrix_ms > 0 and reduce_ms > 0
    opts(time_kernels=0)
    assert raw_bytes(kset, EDGES50, LABELS) == want and ctx.histogram_timing() == (-1.0, -1.0)


def test_distance_distribution_tsv(kset):
    """processors.distance_distribution: its text equals a table built from hist_ref."""
    from gdist import java_double, processors
    D = R.recipe()[3]
    ids = [f"83333.{i}" for i in range(N)]
    groupings = {name: {ids[i]: f"grp{LABELS[t, i]}" for i in range(N) if LABELS[t, i] >= 0}
                 for t, name in enumerate(TYPES)}
    for upper, buckets in ((True, 50), (False, 50), (True, 7)):
        edges = [i / buckets for i in range(buckets + 1)]
        counts, nans, bad = H.hist_ref(D, edges, LABELS, upper=upper)
        out = io.StringIO()
        assert processors.distance_distribution(kset, ids, groupings, out, "recipe.tbl", buckets=buckets,
                                                upper=upper) == int(bad.sum())
        lines = ["dist_file\tgroup_type\tin_out\tlow\thigh\tcount"]
        for t in range(4):
            for k in range(2):
                assert counts[2 * t + k, 0] == 0
                for b in range(1, buckets + 2):
                    high = java_double(edges[b]) if b <= buckets else ""
                    lines.append("\t".join(["recipe.tbl", TYPES[t], ("in", "out")[k], java_double(edges[b - 1]), high,
                                            str(int(counts[2 * t + k, b]))]))
        assert out.getvalue() == "\n".join(lines) + "\n"
        assert len(lines) == 1 + 8 * (buckets + 1)
    assert "recipe.tbl\tone\tin\t1.0\t\t7287\n" in out.getvalue()
    assert "recipe.tbl\tsolo\tin\t0.0\t" + java_double(1 / 7) + "\t0\n" in out.getvalue()
    out2 = io.StringIO()
    processors.distance_distribution(kset, ids, groupings, out2, "recipe.tbl", buckets=7, header=False)
    assert out2.getvalue() == "".join(out.getvalue().splitlines(True)[1:])
    with pytest.raises(ValueError):
        processors.distance_distribution(kset, ids[:-1], groupings, out2, "recipe.tbl")
