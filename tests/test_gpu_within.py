"""Every pair within a distance on the device (gdist_within): the documented
maxDist filter of GenomeProcessor.java:35 as a CSR list. Every answer is
compared with `==` (row pointers, columns, fp64 bits of the distances) against
a filter of the oracle's distance matrix (within_ref), whatever the method, the
row block, the region and the capacity. The outputs are pre-filled with
garbage, so a slot the call leaves unwritten fails and a slot past the
capacity that it touches fails too. Each property of the fixture a test relies
on is asserted on the oracle's matrix first.

Not covered: the EINVAL for 2^32 - 1 sets or more (no such collection fits a test)."""
import ctypes as C
import io

import numpy as np
import pytest

import closest_ref as CR
import oracle
import within_ref as R

pytestmark = pytest.mark.gpu

N = 195
EMPTY_NAN, SKETCH_JACCARD, UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF = 0x400, 0x800, 0x100, 0x200, 0x1000
GARBAGE_I, GARBAGE_D = 0x5A5A5A5A5A5A5A5A, 7.5
THRESHOLDS = (0.0, 0.5, 0.9, 0.97, 1.0)
PAIRS = {0.0: 8, 0.5: 418, 0.9: 10696, 0.97: 22104, 1.0: 37830}


def raw_within(sets, max_dist, rows=None, cols=None, method=0, flags=0, capacity=None, null=()):
    """gdist_within into garbage-filled outputs: (rc, rowptr[nr + 1], cols[cap],
    d[cap], total). capacity None: room for every pair of the region. `null`:
    the outputs handed over as NULL (of "rowptr", "cols", "d", "total")."""
    from gdist import _lib as L
    ns = len(sets)
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    nr = max(r1 - r0, 0)
    cap = max(nr, 0) * max(c1 - c0, 0) if capacity is None else capacity
    rowptr = np.full(nr + 1, GARBAGE_I, dtype=np.int64)
    col = np.full(max(cap, 0) + 3, GARBAGE_I, dtype=np.int64)      # 3 guard slots past the capacity
    d = np.full(max(cap, 0) + 3, GARBAGE_D, dtype=np.float64)
    total = C.c_int64(-9)
    rc = L.lib.gdist_within(sets.ctx.h, sets.h, r0, r1, c0, c1, method, flags, max_dist, cap,
                            None if "rowptr" in null else L.ptr(rowptr, C.c_int64),
                            None if "cols" in null else L.ptr(col, C.c_int64),
                            None if "d" in null else L.ptr(d, C.c_double),
                            None if "total" in null else C.byref(total))
    return rc, rowptr, col, d, total.value


def check(sets, D, max_dist, rows=None, cols=None, method=0, flags=0, capacity=None, null=()):
    """The call equals within_ref on D (the oracle's matrix of the whole
    collection): the row pointers and the total whole, the first min(total,
    capacity) entries, and garbage after them. Returns (rowptr, cols, d) cut to
    the entries written."""
    ns = D.shape[0]
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    rc, rowptr, col, d, total = raw_within(sets, max_dist, rows, cols, method, flags, capacity, null)
    assert rc == 0
    erow, ecol, ed = R.within_ref(D[r0:r1, c0:c1], max_dist, r0, c0, upper=bool(flags & UPPER_TRIANGLE),
                                  keep_self=bool(flags & KEEP_SELF))
    assert np.array_equal(rowptr, erow)
    assert total == erow[-1]
    m = min(total, len(col) - 3)
    assert np.array_equal(col[:m], ecol[:m])
    assert np.array_equal(d[:m].view(np.uint64), ed[:m].view(np.uint64))
    assert np.all(col[m:] == GARBAGE_I) and np.all(d[m:] == GARBAGE_D)
    return rowptr, col[:m], d[:m]


def same_bytes(a, b):
    return all(np.array_equal(x.view(np.uint8), y.view(np.uint8)) for x, y in zip(a, b))


@pytest.fixture(scope="module")
def kset(ctx):
    import gdist
    seqs, _, _, D = CR.recipe()
    assert D.shape == (N, N)
    s = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


def test_fixture_properties():
    """What the tests below rely on, on the oracle's matrix (off-diagonal ordered pairs)."""
    _, off, _, D = CR.recipe()
    offd = ~np.eye(N, dtype=bool)
    for md, pairs in PAIRS.items():
        ok = (D <= md) & offd
        assert int(ok.sum()) == pairs
        assert int(np.triu(ok, 1).sum()) * 2 == pairs               # the upper triangle holds half
    assert PAIRS[1.0] == N * (N - 1)
    per_row = ((D <= 0.9) & offd).sum(1)
    assert int((per_row == 0).sum()) == 45 and int((per_row > 64).sum()) == 76 and int(per_row.max()) == 149
    assert np.diff(off)[-2:].tolist() == [0, 0]                     # two empty sets
    assert not np.isnan(D).any()


@pytest.mark.parametrize("method", [1, 2, 0], ids=["sorted", "bitset", "auto"])
@pytest.mark.parametrize("max_dist", THRESHOLDS)
def test_methods_and_thresholds(kset, method, max_dist):
    D = CR.recipe()[3]
    got = check(kset, D, max_dist, method=method)
    assert len(got[1]) == PAIRS[max_dist]
    again = raw_within(kset, max_dist, method=method)
    assert again[0] == 0 and again[4] == PAIRS[max_dist]
    assert same_bytes(got, (again[1], again[2][:again[4]], again[3][:again[4]]))


@pytest.mark.parametrize("rows_", [1, 7, 64, 128])
def test_row_blocks(kset, opts, rows_):
    """Several row blocks with a ragged last one: the bytes do not depend on closest_rows."""
    D = CR.recipe()[3]
    assert N % rows_ != 0 or rows_ == 1
    base = check(kset, D, 0.9)
    opts(closest_rows=rows_)
    for method in (1, 2):
        assert same_bytes(base, check(kset, D, 0.9, method=method))
    assert same_bytes(check(kset, D, 1.0), R.within_ref(D, 1.0))


def test_rectangles(kset, opts):
    D = CR.recipe()[3]
    for method in (1, 2):
        got = check(kset, D, 0.9, rows=(3, 131), cols=(60, 193), method=method)       # the rows' own columns inside
        assert 0 < len(got[1]) < 128 * 133
        got = check(kset, D, 0.9, rows=(150, 195), cols=(0, 150), method=method)      # disjoint: M x N use
        assert 0 < len(got[1]) < 45 * 150
    # column ranges below, at and above one 64-column load, and of one column
    for width in (1, 63, 64, 65):
        for c0 in (0, 5, N - width):
            check(kset, D, 0.9, cols=(c0, c0 + width))
            check(kset, D, 1.0, rows=(0, 70), cols=(c0, c0 + width), flags=KEEP_SELF)
    opts(closest_rows=16)
    check(kset, D, 1.0, rows=(3, 131), cols=(60, 193))


def test_sharding(kset):
    """Disjoint row ranges concatenate: shift the later rowptr, no merge."""
    D = CR.recipe()[3]
    full = check(kset, D, 0.9)
    rowptr, cols, d = [np.zeros(1, np.int64)], [], []
    for rows in ((0, 50), (50, 131), (131, 195)):
        rp, c, dd = check(kset, D, 0.9, rows=rows)
        rowptr.append(rp[1:] + rowptr[-1][-1])
        cols.append(c)
        d.append(dd)
    assert same_bytes(full, (np.concatenate(rowptr), np.concatenate(cols), np.concatenate(d)))


def test_upper(kset, opts):
    D = CR.recipe()[3]
    for block in (None, 16):
        if block:
            opts(closest_rows=block)
        for method in (1, 2):
            for max_dist in THRESHOLDS:
                rowptr, cols, d = check(kset, D, max_dist, method=method, flags=UPPER_TRIANGLE)
                assert len(cols) * 2 == PAIRS[max_dist]
                # the full answer filtered to j > i
                frow, fcols, fd = check(kset, D, max_dist, method=method)
                keep = fcols > np.repeat(np.arange(N), np.diff(frow))
                assert np.array_equal(cols, fcols[keep]) and np.array_equal(d.view(np.uint64), fd[keep].view(np.uint64))
        # KEEP_SELF adds nothing under upper; a rectangle left of, across and right of the diagonal
        assert same_bytes(check(kset, D, 0.9, flags=UPPER_TRIANGLE | KEEP_SELF), check(kset, D, 0.9, flags=UPPER_TRIANGLE))
        assert check(kset, D, 1.0, rows=(100, 195), cols=(0, 100), flags=UPPER_TRIANGLE)[0][-1] == 0
        check(kset, D, 1.0, rows=(20, 150), cols=(60, 130), flags=UPPER_TRIANGLE)
        assert check(kset, D, 1.0, rows=(0, 60), cols=(60, 195), flags=UPPER_TRIANGLE)[0][-1] == 60 * 135


def test_self(kset):
    D = CR.recipe()[3]
    rowptr, cols, d = check(kset, D, 0.0, flags=KEEP_SELF)
    lists = R.as_lists(rowptr, cols, d)
    # a set is at 0.0 from itself; sets 150, 151 repeat set 5 and set 152 repeats set 77:
    # the duplicates appear in column order. The empty sets are at 1.0 from themselves.
    dups = {5: [5, 150, 151], 150: [5, 150, 151], 151: [5, 150, 151], 77: [77, 152], 152: [77, 152]}
    for q in range(N):
        want = dups.get(q, [q]) if q < N - 2 else []
        assert lists[q] == [(j, 0.0) for j in want], q
    assert rowptr[-1] == 193 + PAIRS[0.0]
    rowptr9, _, _ = check(kset, D, 0.9, flags=KEEP_SELF)
    assert rowptr9[-1] == PAIRS[0.9] + 193
    assert check(kset, D, 1.0, flags=KEEP_SELF)[0][-1] == N * N


@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["default", "empty_nan"])
def test_empty_sets(kset, flags):
    """Two empty sets: at 1.0 from everything by default (listed from max_dist
    1.0 on), NaN from each other and themselves with EMPTY_NAN (never listed)."""
    _, off, codes, _ = CR.recipe()
    _, D = oracle.matrix(off, codes, 0, N, 0, N, flags=flags)
    assert int(np.isnan(D).sum()) == (4 if flags else 0)
    for method in (1, 2):
        rowptr, cols, d = check(kset, D, 1.0, method=method, flags=flags)
        assert np.diff(rowptr)[N - 2:].tolist() == ([N - 2, N - 2] if flags else [N - 1, N - 1])
        assert not np.isnan(d).any()
        rowptr, cols, d = check(kset, D, 1.0, method=method, flags=flags | KEEP_SELF)
        assert np.diff(rowptr)[N - 2:].tolist() == ([N - 2, N - 2] if flags else [N, N])
        assert rowptr[-1] == N * N - (4 if flags else 0) and not np.isnan(d).any()
        rowptr, _, _ = check(kset, D, 0.99, method=method, flags=flags)
        assert np.diff(rowptr)[N - 2:].tolist() == [0, 0]


def test_capacity(kset, opts):
    """The counting call, the exact total, one less, and a cut in the middle of a row."""
    D = CR.recipe()[3]
    erow = R.within_ref(D, 0.9)[0]
    total = int(erow[-1])
    assert total == PAIRS[0.9]
    k = int(np.flatnonzero(np.diff(erow) >= 2)[3])
    mid = int(erow[k]) + 1
    assert erow[k] < mid < erow[k + 1] and k > 0
    for block in (None, 7):
        if block:
            opts(closest_rows=block)
        for method in (1, 2):
            rowptr, cols, d = check(kset, D, 0.9, method=method, capacity=0, null=("cols", "d"))
            assert len(cols) == 0 and rowptr[-1] == total
            check(kset, D, 0.9, method=method, capacity=0)                      # non-null arrays stay untouched
            for cap in (total, total - 1, mid, 1, total + 5):
                rowptr, cols, d = check(kset, D, 0.9, method=method, capacity=cap)
                assert len(cols) == min(cap, total) and rowptr[-1] == total
        check(kset, D, 0.9, flags=UPPER_TRIANGLE, capacity=mid)
        check(kset, D, 0.9, rows=(3, 131), cols=(60, 193), capacity=100)


def test_rows_longer_than_one_tile(ctx, opts):
    """1,100 columns: a row is three tiles of the kernels (512 columns each), the
    last one ragged (76 columns: one full 64-column load and 12 lanes of the
    next), so positions come from the scan across the tiles of a row. The
    recipe's 195 columns fit one tile."""
    import gdist
    from gdist import synth
    n = 1100
    seqs = [bytes(r) for r in synth.genomes(n, 150, 0.03, 51)]
    off, codes = oracle.pack(seqs, 15, 0, 0)
    _, D = oracle.matrix(off, codes, 0, n, 0, n)
    per_row = ((D <= 0.5) & ~np.eye(n, dtype=bool)).sum(1)
    assert int(per_row.sum()) == 488858 and per_row.min() == 0 and per_row.max() == 931
    s = gdist.KmerSets.from_sequences(seqs, 15, gdist.KmerType.DNA, 0, ctx)
    erow = R.within_ref(D, 0.5)[0]
    k = int(np.argmax(per_row))
    for method in (1, 2):
        base = check(s, D, 0.5, method=method)
        check(s, D, 0.5, method=method, flags=UPPER_TRIANGLE)
        check(s, D, 0.5, method=method, capacity=int(erow[k]) + 700)          # cut in the row's second tile
        check(s, D, 0.5, method=method, rows=(100, 400), cols=(7, 1036))     # 1,029 columns: two tiles and 5 columns
        check(s, D, 1.0, method=method, rows=(500, 600), flags=KEEP_SELF)
    opts(closest_rows=100)
    assert same_bytes(base, check(s, D, 0.5))
    check(s, D, 0.5, flags=UPPER_TRIANGLE, capacity=int(erow[k]) // 2 + 3)
    s.free()


def test_python_api(kset, monkeypatch):
    import gdist
    D = CR.recipe()[3]
    want = R.within_ref(D, 0.9)
    got = kset.within(0.9)
    assert [a.dtype for a in got] == [np.int64, np.int64, np.float64]
    assert got[0].shape == (N + 1,) and got[1].shape == got[2].shape == (PAIRS[0.9],)
    assert same_bytes(got, want)
    # a first guess that is too small: the second call completes the answer
    monkeypatch.setattr(gdist.KmerSets, "WITHIN_GUESS_PER_ROW", 1)
    assert N < PAIRS[0.9]
    assert same_bytes(kset.within(0.9), want)
    assert same_bytes(kset.within(0.9, upper=True, method=gdist.METHOD_SORTED), R.within_ref(D, 0.9, upper=True))
    # a number: at most that many entries, rowptr still the full counts
    rowptr, cols, d = kset.within(0.9, capacity=100)
    assert np.array_equal(rowptr, want[0]) and same_bytes((cols, d), (want[1][:100], want[2][:100]))
    rowptr, cols, d = kset.within(0.9, capacity=0)
    assert np.array_equal(rowptr, want[0]) and len(cols) == len(d) == 0
    got = kset.within(0.5, rows=(3, 131), cols=(60, 193), keep_self=True, method=gdist.METHOD_BITSET)
    assert same_bytes(got, R.within_ref(D[3:131, 60:193], 0.5, 3, 60, keep_self=True))
    with pytest.raises(ValueError):
        kset.within(0.9, capacity=-1)
    with pytest.raises(ValueError):
        kset.within(float("nan"))


def test_protein(ctx):
    import gdist
    from gdist import synth
    prots = [bytes(r) for r in synth.genomes(60, 400, 0.1, 43, protein=True)]
    off, codes = oracle.pack(prots, 8, 1, 0)
    _, D = oracle.matrix(off, codes, 0, 60, 0, 60)
    offd = ~np.eye(60, dtype=bool)
    # every pair of this recipe lies within 0.97; 0.8 cuts the rows in the middle
    assert int(((D <= 0.97) & offd).sum()) == 60 * 59 and int(((D <= 0.8) & offd).sum()) == 2828
    s = gdist.KmerSets.from_sequences(prots, 8, gdist.KmerType.PROT, 0, ctx)
    for method in (1, 2):
        assert check(s, D, 0.97, method=method)[0][-1] == 60 * 59
        assert check(s, D, 0.8, method=method)[0][-1] == 2828
        check(s, D, 0.8, method=method, flags=UPPER_TRIANGLE)
    s.free()


@pytest.fixture(scope="module")
def sketch_case(ctx):
    """The first 120 sequences of the recipe and one of 100 bp (a dwarf at
    width 200); per width the collection and the oracle's signatures."""
    import gdist
    from gdist import synth
    seqs = CR.recipe_sequences()[:120] + [bytes(synth.genomes(1, 100, 0.0, 7)[0])]
    off, codes = oracle.pack(seqs, 21, 0, 0)
    ks = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    out = {}
    for width in (64, 200):
        sigs = [oracle.sketch(codes[off[i]:off[i + 1]], 21, 0, width) for i in range(len(seqs))]
        out[width] = (ks.sketches(width), sigs)
    assert len(out[200][1][120]) < 200 and len(out[64][1][120]) == 64
    yield out
    for sk, _ in out.values():
        sk.free()
    ks.free()


@pytest.mark.parametrize("flags", [0, SKETCH_JACCARD], ids=["mash", "jaccard"])
@pytest.mark.parametrize("width", [64, 200])
def test_sketches(sketch_case, opts, width, flags):
    sk, sigs = sketch_case[width]
    m = len(sigs)
    D = np.array([[oracle.sketch_distance(sigs[i], sigs[j], width, flags)[0] for j in range(m)] for i in range(m)])
    n9 = int(((D <= 0.9) & ~np.eye(m, dtype=bool)).sum())
    assert 0 < n9 < m * (m - 1)
    base = check(sk, D, 0.9, flags=flags)
    assert len(base[1]) == n9
    assert same_bytes(base, check(sk, D, 0.9, method=77, flags=flags))      # the method argument is ignored
    check(sk, D, 1.0, flags=flags | KEEP_SELF)
    check(sk, D, 0.9, flags=flags | UPPER_TRIANGLE)
    check(sk, D, 0.9, flags=flags, capacity=n9 // 2)
    opts(closest_rows=50)
    assert same_bytes(base, check(sk, D, 0.9, flags=flags))
    check(sk, D, 0.9, rows=(100, 121), cols=(0, 100), flags=flags)
    got = sk.within(0.9, rows=(100, 121), cols=(0, 100), flags=flags)
    assert same_bytes(got, R.within_ref(D[100:121, 0:100], 0.9, 100, 0))
    # upper, still 50 rows a block: rows 60..109 straddle the diagonal of the
    # columns (0, 100), rows 110..120 lie wholly left of it and have no step
    cut = check(sk, D, 0.9, rows=(60, 121), cols=(0, 100), flags=flags | UPPER_TRIANGLE)
    assert 0 < cut[0][50] and np.all(cut[0][50:] == cut[0][50])
    opts(closest_rows=None)
    assert same_bytes(cut, check(sk, D, 0.9, rows=(60, 121), cols=(0, 100), flags=flags | UPPER_TRIANGLE))


def test_errors_and_edge_cases(kset, ctx):
    import gdist
    from gdist import _lib as L
    D = CR.recipe()[3]

    def einval(*a, **kw):
        rc, rowptr, col, d, total = raw_within(*a, **kw)
        assert rc == L.EINVAL and L.lib.gdist_last_error()
        # refused before any work: the outputs keep the caller's values
        assert np.all(rowptr == GARBAGE_I) and np.all(col == GARBAGE_I) and np.all(d == GARBAGE_D) and total == -9

    einval(kset, 0.9, rows=(0, N + 1))
    einval(kset, 0.9, rows=(-1, 5))
    einval(kset, 0.9, rows=(9, 5), capacity=10)
    einval(kset, 0.9, cols=(0, N + 1))
    einval(kset, 0.9, cols=(7, 3), capacity=10)
    einval(kset, float("nan"))
    einval(kset, 0.9, capacity=-1)
    einval(kset, 0.9, null=("rowptr",))
    einval(kset, 0.9, null=("total",))
    einval(kset, 0.9, capacity=10, null=("cols",))
    einval(kset, 0.9, capacity=10, null=("d",))
    einval(kset, 0.9, flags=OUT_DEVICE)
    einval(kset, 0.9, method=3)
    einval(kset, 0.9, method=-1)
    rowptr, col, d = np.zeros(3, np.int64), np.zeros(4, np.int64), np.zeros(4)
    total = C.c_int64(0)
    out = (L.ptr(rowptr, C.c_int64), L.ptr(col, C.c_int64), L.ptr(d, C.c_double), C.byref(total))
    assert L.lib.gdist_within(ctx.h, None, 0, 2, 0, 2, 0, 0, 0.9, 4, *out) == L.EINVAL      # null collection
    assert L.lib.gdist_within(None, kset.h, 0, 2, 0, 2, 0, 0, 0.9, 4, *out) == L.EINVAL     # null context
    # a bitsets-only collection: SORTED is refused, BITSET and AUTO answer
    seqs = CR.recipe_sequences()
    b = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    b.build_bitsets()
    b.release_codes()
    einval(b, 0.9, method=1)
    assert check(b, D, 0.9, method=2)[0][-1] == PAIRS[0.9]
    assert check(b, D, 0.9, method=0)[0][-1] == PAIRS[0.9]
    b.free()
    # empty ranges: OK, zero row pointers, total 0, nothing written
    rc, rowptr, col, d, total = raw_within(kset, 0.9, rows=(5, 5), capacity=4)
    assert rc == 0 and rowptr.tolist() == [0] and total == 0 and np.all(col == GARBAGE_I) and np.all(d == GARBAGE_D)
    rc, rowptr, col, d, total = raw_within(kset, 0.9, rows=(5, 9), cols=(20, 20), capacity=4)
    assert rc == 0 and rowptr.tolist() == [0] * 5 and total == 0 and np.all(col == GARBAGE_I)
    rc, rowptr, col, d, total = raw_within(kset, 0.9, rows=(5, 5), cols=(20, 20), capacity=0, null=("cols", "d"))
    assert rc == 0 and rowptr.tolist() == [0] and total == 0
    prow, pcol, pd = kset.within(0.9, rows=(5, 5))
    assert prow.tolist() == [0] and len(pcol) == len(pd) == 0
    # thresholds outside [0, 1]: nothing below a negative one, everything but NaN under +inf
    assert check(kset, D, -1.0)[0].tolist() == [0] * (N + 1)
    assert check(kset, D, -1.0, flags=KEEP_SELF)[0][-1] == 0
    assert check(kset, D, float("inf"))[0][-1] == N * (N - 1)
    _, off, codes, _ = CR.recipe()
    _, Dn = oracle.matrix(off, codes, 0, N, 0, N, flags=EMPTY_NAN)
    assert check(kset, Dn, float("inf"), flags=EMPTY_NAN | KEEP_SELF)[0][-1] == N * N - 4


def test_timing(kset, ctx, opts):
    D = CR.recipe()[3]
    base = check(kset, D, 0.9)
    assert ctx.within_timing() == (-1.0, -1.0)
    opts(time_kernels=1)
    for method in (1, 2):
        assert same_bytes(base, check(kset, D, 0.9, method=method))
        m, s = ctx.within_timing()
        assert m >= 0.0 and s >= 0.0
    opts(closest_rows=64)
    assert same_bytes(base, check(kset, D, 0.9, capacity=0, null=("cols", "d"))[:1])
    m, s = ctx.within_timing()
    assert m >= 0.0 and s >= 0.0
    opts(time_kernels=0)
    check(kset, D, 0.9)
    assert ctx.within_timing() == (-1.0, -1.0)


def test_processors(ctx):
    """fasta_close_pairs: the fastaDist lines with d <= max_dist from the
    oracle's matrix; genome_distance(within=True): its within=False output with
    the lines above max_dist dropped. In both some but not all lines survive."""
    import gdist
    from gdist import processors
    from gdist.javafmt import java_double
    seqs, _, _, D = CR.recipe()
    pick = list(range(0, 24)) + [150, 151, 152, 77, 100] + list(range(153, 163)) + [193]
    assert len(pick) == 40
    recs = [gdist.Sequence(f"s{i}", f"genome {i}", seqs[i].decode()) for i in pick]
    sub = D[np.ix_(pick, pick)]
    for max_dist in (0.9, 0.0):
        lines = ["seq1\tname1\tseq2\tname2\tdistance"]
        for a in range(40):
            for b in range(a + 1, 40):
                if sub[a, b] <= max_dist:
                    lines.append(f"s{pick[a]}\tgenome {pick[a]}\ts{pick[b]}\tgenome {pick[b]}\t{java_double(sub[a, b])}")
        assert 1 < len(lines) < 1 + 40 * 39 // 2
        out = io.StringIO()
        assert processors.fasta_close_pairs(recs, out, max_dist, kmer_size=21, ctx=ctx) == len(lines) - 1
        assert out.getvalue() == "\n".join(lines) + "\n"
    # the same lines fasta_distance writes, filtered
    out = io.StringIO()
    processors.fasta_distance(recs, out, kmer_size=21, ctx=ctx)
    every = out.getvalue().splitlines()
    keep = [sub[a, b] <= 0.9 for a in range(40) for b in range(a + 1, 40)]
    out = io.StringIO()
    processors.fasta_close_pairs(recs, out, 0.9, kmer_size=21, ctx=ctx)
    assert out.getvalue().splitlines() == every[:1] + [ln for ln, k in zip(every[1:], keep) if k]
    with pytest.raises(processors.ParseFailureException):
        processors.fasta_close_pairs(recs, io.StringIO(), 0.9, kmer_size=1, ctx=ctx)
    out = io.StringIO()
    assert processors.fasta_close_pairs(recs[:1], out, 0.9, kmer_size=21, ctx=ctx) == 0
    assert out.getvalue() == every[0] + "\n"

    mk = lambda i: processors.Genome(f"83333.{i}", f"Genome number {i}", [seqs[i].decode()])
    base_i = list(range(0, 30)) + [193, 160]
    comp_i = [[150, 136, 5], [160, 194, 147, 77, 152, 141]]
    base, others = [mk(i) for i in base_i], [[mk(i) for i in grp] for grp in comp_i]
    flat = [i for grp in comp_i for i in grp]
    out = io.StringIO()
    assert processors.genome_distance(base, others, out, ctx=ctx) == len(flat) * len(base_i)
    every = out.getvalue().splitlines()
    for max_dist in (0.9, 1.0, 0.5):
        keep = [D[q, b] <= max_dist for q in flat for b in base_i]
        if max_dist < 1.0:
            assert 0 < sum(keep) < len(keep)
        out = io.StringIO()
        assert processors.genome_distance(base, others, out, max_dist=max_dist, ctx=ctx, within=True) == sum(keep)
        assert out.getvalue().splitlines() == every[:1] + [ln for ln, k in zip(every[1:], keep) if k]
    assert "\t0.0" in "\n".join(every)                      # genome 5 against base genome 5


def test_jni_within(kset, tmp_path_factory):
    """nWithin through the shim equals the Python path; arrays shorter than the
    total get their length and the total comes back; a null collection is an
    IllegalArgumentException."""
    from jni_harness import harness
    from jni_harness.harness import LONG, DOUBLE
    jvm = harness.FakeJVM(harness.current() or
                          harness.build(str(tmp_path_factory.mktemp("jni") / "libgdist_jni_test.so")))
    seqs = CR.recipe_sequences()
    sig = [C.c_int64] * 6 + [C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    ctx = jvm.call_i("nCtxCreate", C.c_int64, [C.c_int32], 0)
    sets = jvm.call_i("nPack", C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
                      ctx, 0, 21, 0, jvm.byte_arrays(seqs))
    assert jvm.exception() is None and sets
    for (r0, r1, c0, c1, md, fl) in ((0, N, 0, N, 0.9, 0), (150, N, 0, 150, 1.0, 0), (0, 20, 0, N, 0.9, KEEP_SELF),
                                     (0, N, 0, N, 0.9, UPPER_TRIANGLE)):
        nr = r1 - r0
        prow, pcol, pd = kset.within(md, rows=(r0, r1), cols=(c0, c1), upper=bool(fl & UPPER_TRIANGLE),
                                     keep_self=bool(fl & KEEP_SELF))
        total = int(prow[-1])
        assert total > 8
        for cap in (total + 2, total // 2):
            jr = jvm.array(LONG, [7] * (nr + 1))
            jc, jd = jvm.array(LONG, [7] * cap), jvm.array(DOUBLE, [7.5] * (cap + 1))     # capacity: the shorter one
            assert jvm.call_i("nWithin", C.c_int64, sig, ctx, sets, r0, r1, c0, c1, 0, fl, md, jr, jc, jd) == total
            assert jvm.exception() is None
            m = min(total, cap)
            assert jvm.read(jr, LONG, nr + 1) == prow.tolist()
            assert jvm.read(jc, LONG, cap) == pcol[:m].tolist() + [7] * (cap - m)
            got = np.array(jvm.read(jd, DOUBLE, cap + 1))
            assert np.array_equal(got[:m].view(np.uint64), pd[:m].view(np.uint64)) and np.all(got[m:] == 7.5)
    jr, jc, jd = jvm.zeros(LONG, 3), jvm.zeros(LONG, 20), jvm.zeros(DOUBLE, 20)
    assert jvm.call_i("nWithin", C.c_int64, sig, ctx, 0, 0, 2, 0, 2, 0, 0, 0.9, jr, jc, jd) == 0   # a null collection
    cls, msg = jvm.exception()
    assert cls == "java/lang/IllegalArgumentException" and msg
    jvm.call_i("nWithin", C.c_int64, sig, ctx, sets, 0, 2, 0, 2, 0, 0, 0.9, jvm.zeros(LONG, 2), jc, jd)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "rowptr shorter than r1 - r0 + 1")
    jvm.call_i("nWithin", C.c_int64, sig, ctx, sets, 5, 2, 0, 2, 0, 0, 0.9, jr, jc, jd)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "negative row range")
    jvm.call_i("nWithin", C.c_int64, sig, ctx, sets, 0, 2, 0, N + 1, 0, 0, 0.9, jr, jc, jd)
    assert jvm.exception()[0] == "java/lang/IllegalArgumentException"                     # a bad column range
    jvm.call_i("nWithin", C.c_int64, sig, ctx, sets, 0, 2, 0, 2, 0, 0, 0.9, jr, None, jd)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "null cols")
    jvm.call("nFree", None, sets)
    jvm.call("nCtxDestroy", None, ctx)
    assert jvm.exception() is None
