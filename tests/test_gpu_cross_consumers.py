"""The three table-free queries against a resident collection on the device
(gdist_cross_within, gdist_cross_group_stats, gdist_cross_histogram): the
comparison genomes of the genomes table against pre-loaded base genomes
(GenomeProcessor.java:35,140), the distCheck and taxCheck summaries of new
genomes against a database. Every answer is compared bit for bit: integer
outputs with array_equal, d through its uint64 view, group sides field by field
(group_ref.check_stats) and as bytes against the one-collection twin on
gdist_sets_concat(subjects, queries) with METHOD_SORTED. Outputs are pre-filled
with poison, so an entry the call leaves unwritten, or writes past its
capacity, fails. Not covered: a subject collection of 2^32 - 1 sets (it does
not fit a test)."""
import ctypes as C
import io
import types

import numpy as np
import pytest

import cross_consumers_ref as Z
import cross_ref as X
import group_ref as G
import hist_ref as H
import oracle
import within_ref as W

pytestmark = pytest.mark.gpu

EMPTY_NAN, UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF = 0x400, 0x100, 0x200, 0x1000
POISON_RP, POISON_COL, POISON_D, POISON_CNT, POISON_BYTE = -77, 0x5A5A5A5A5A5A5A5A, 7.5, -9, 0x5A
NS, NQ = Z.NS, Z.NQ
INF = float("inf")


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


# ---- raw calls into poisoned outputs ---------------------------------------
def raw_within(subj, qry, max_dist, rows=None, cols=None, flags=0, capacity=None, null_lists=False, ctx=None,
               null_rowptr=False, null_total=False):
    """(rc, rowptr[nr + 1], col[cap + 8], d[cap + 8], total): capacity None asks
    for every cell of the rectangle; the arrays are 8 entries longer than the
    capacity the call is given."""
    from gdist import _lib as L
    r0, r1 = rows or (0, len(qry))
    c0, c1 = cols or (0, len(subj))
    nr = max(r1 - r0, 0)
    cap = nr * max(c1 - c0, 0) if capacity is None else capacity
    rowptr = np.full(nr + 1, POISON_RP, dtype=np.int64)
    col = np.full(max(cap, 0) + 8, POISON_COL, dtype=np.int64)
    d = np.full(max(cap, 0) + 8, POISON_D, dtype=np.float64)
    total = C.c_int64(POISON_CNT)
    rc = L.lib.gdist_cross_within((ctx or subj.ctx).h, qry.h, subj.h, r0, r1, c0, c1, flags, max_dist, cap,
                                  None if null_rowptr else L.ptr(rowptr, C.c_int64),
                                  None if null_lists else L.ptr(col, C.c_int64),
                                  None if null_lists else L.ptr(d, C.c_double),
                                  None if null_total else C.byref(total))
    return rc, rowptr, col, d, total.value


def raw_group(subj, qry, rows=None, cols=None, flags=0, qlab=Z.QLABELS, slab=Z.SLABELS, ntypes=None, ctx=None,
              null=()):
    """(rc, sides bytes [2 T] as uint8, bad[T]) of gdist_cross_group_stats."""
    from gdist import _lib as L
    r0, r1 = rows or (0, len(qry))
    c0, c1 = cols or (0, len(subj))
    T = len(qlab) if ntypes is None else ntypes
    sides = np.full(2 * max(T, 1) * C.sizeof(L.GroupSide), POISON_BYTE, dtype=np.uint8)
    bad = np.full(max(T, 1), POISON_CNT, dtype=np.int64)
    ql, sl = np.ascontiguousarray(qlab, dtype=np.int32), np.ascontiguousarray(slab, dtype=np.int32)
    rc = L.lib.gdist_cross_group_stats((ctx or subj.ctx).h, qry.h, subj.h, r0, r1, c0, c1, flags, T,
                                       None if "qlabels" in null else L.ptr(ql, C.c_int32),
                                       None if "slabels" in null else L.ptr(sl, C.c_int32),
                                       None if "out" in null else sides.ctypes.data,
                                       None if "bad" in null else L.ptr(bad, C.c_int64))
    return rc, sides, bad


def as_sides(raw):
    from gdist import _lib as L
    return (L.GroupSide * (len(raw) // C.sizeof(L.GroupSide))).from_buffer_copy(raw.tobytes())


def raw_hist(subj, qry, edges, rows=None, cols=None, flags=0, labelled=True, ntypes=None, nedges=None, ctx=None,
             null=()):
    """(rc, counts[S, E + 1], nans[S], bad[T]) of gdist_cross_histogram."""
    from gdist import _lib as L
    r0, r1 = rows or (0, len(qry))
    c0, c1 = cols or (0, len(subj))
    e = np.ascontiguousarray(edges, dtype=np.float64)
    E = len(e) if nedges is None else nedges
    T = (Z.NTYPES if labelled else 0) if ntypes is None else ntypes
    S = 2 * T if T > 0 else 1
    counts = np.full((S, max(E, 0) + 1), POISON_CNT, dtype=np.int64)
    nans = np.full(S, POISON_CNT, dtype=np.int64)
    bad = np.full(max(T, 1), POISON_CNT, dtype=np.int64)
    ql, sl = np.ascontiguousarray(Z.QLABELS), np.ascontiguousarray(Z.SLABELS)
    rc = L.lib.gdist_cross_histogram((ctx or subj.ctx).h, qry.h, subj.h, r0, r1, c0, c1, flags, E,
                                     None if "edges" in null else L.ptr(e, C.c_double), T,
                                     L.ptr(ql, C.c_int32) if labelled and "qlabels" not in null else None,
                                     L.ptr(sl, C.c_int32) if labelled and "slabels" not in null else None,
                                     None if "counts" in null else L.ptr(counts, C.c_int64),
                                     None if "nans" in null else L.ptr(nans, C.c_int64),
                                     L.ptr(bad, C.c_int64) if labelled and "bad" not in null else None)
    return rc, counts, nans, bad


# ---- checks against the refs -------------------------------------------------
def check_within(subj, qry, max_dist, flags=0, rows=None, cols=None):
    rc, rowptr, col, d, total = raw_within(subj, qry, max_dist, rows, cols, flags)
    assert rc == 0
    erp, ecol, ed = Z.within_expected(max_dist, flags, rows, cols)
    assert np.array_equal(rowptr, erp) and total == erp[-1] == len(ecol)
    assert np.array_equal(col[:total], ecol)
    assert np.array_equal(bits(d[:total]), bits(ed))
    assert np.all(col[total:] == POISON_COL) and np.all(d[total:] == POISON_D)   # the tail past the total
    return rowptr, col[:total], d[:total]


def check_group(subj, qry, flags=0, rows=None, cols=None):
    rc, sides, bad = raw_group(subj, qry, rows, cols, flags)
    assert rc == 0
    G.check_stats(as_sides(sides), bad, Z.group_expected(flags, rows, cols), f"rows {rows} cols {cols}")
    return sides.tobytes() + bad.tobytes()


def check_hist(subj, qry, edges, flags=0, rows=None, cols=None, labelled=True):
    rc, counts, nans, bad = raw_hist(subj, qry, edges, rows, cols, flags, labelled)
    assert rc == 0
    ec, en, eb = Z.hist_expected(edges, flags, rows, cols, labelled)
    assert np.array_equal(counts, ec) and np.array_equal(nans, en)
    if labelled:
        assert np.array_equal(bad, eb)
    else:
        assert np.all(bad == POISON_CNT)
    return counts, nans, bad


@pytest.fixture(scope="module")
def subj(ctx):
    import gdist
    Z.check_fixture()
    s = gdist.KmerSets.from_sequences(X.sequences()[0], 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


@pytest.fixture(scope="module")
def qry(ctx):
    import gdist
    s = gdist.KmerSets.from_sequences(X.sequences()[1], 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


@pytest.fixture(scope="module")
def both(subj, qry):
    """gdist_sets_concat(subjects, queries): the collection of the twins."""
    b = subj.concat(qry)
    assert len(b) == NS + NQ
    yield b
    b.free()


# 1 ---- within ----------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["plain", "empty_nan"])
@pytest.mark.parametrize("max_dist", [0.9, 0.0, 1.0, -1.0, INF])
def test_within_thresholds(subj, qry, both, max_dist, flags):
    import gdist
    rowptr, col, d = check_within(subj, qry, max_dist, flags)
    trp, tcol, td = both.within(max_dist, rows=(NS, NS + NQ), cols=(0, NS), method=gdist.METHOD_SORTED,
                                flags=flags, keep_self=True)
    assert rowptr.tobytes() == trp.tobytes() and col.tobytes() == tcol.tobytes() and d.tobytes() == td.tobytes()


def test_within_capacity(subj, qry):
    erp, ecol, ed = Z.within_expected(0.9)
    total = int(erp[-1])
    # the counting call: no list at all
    rc, rowptr, col, d, t = raw_within(subj, qry, 0.9, capacity=0, null_lists=True)
    assert rc == 0 and t == total and np.array_equal(rowptr, erp)
    rc, rowptr, col, d, t = raw_within(subj, qry, 0.9, capacity=0)
    assert rc == 0 and t == total and np.all(col == POISON_COL) and np.all(d == POISON_D)
    # a capacity that cuts a row in the middle
    row = int(np.flatnonzero(np.diff(erp) >= 10)[1])
    cap = int(erp[row]) + 4
    assert erp[row] < cap < erp[row + 1]
    rc, rowptr, col, d, t = raw_within(subj, qry, 0.9, capacity=cap)
    assert rc == 0 and t == total and np.array_equal(rowptr, erp)
    assert np.array_equal(col[:cap], ecol[:cap]) and np.array_equal(bits(d[:cap]), bits(ed[:cap]))
    assert np.all(col[cap:] == POISON_COL) and np.all(d[cap:] == POISON_D)
    # a capacity above the total leaves the tail alone
    rc, rowptr, col, d, t = raw_within(subj, qry, 0.9, capacity=total + 5)
    assert rc == 0 and t == total
    assert np.array_equal(col[:total], ecol) and np.array_equal(bits(d[:total]), bits(ed))
    assert np.all(col[total:] == POISON_COL) and np.all(d[total:] == POISON_D)


# 2 ---- group stats and histogram against refs and twins ------------------------
@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["plain", "empty_nan"])
def test_group_stats_parity(subj, qry, both, flags):
    import gdist
    got = check_group(subj, qry, flags)
    twin = both.group_stats(Z.LABELS, rows=(NS, NS + NQ), cols=(0, NS), upper=False, method=gdist.METHOD_SORTED,
                            flags=flags)
    assert got == twin.tobytes()


HIST_EDGES = {"fifty": lambda: Z.EDGES50, "ulp_inf_one": Z.ulp_edges}


@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["plain", "empty_nan"])
@pytest.mark.parametrize("labelled", [False, True], ids=["one_series", "four_series"])
@pytest.mark.parametrize("edges", sorted(HIST_EDGES))
def test_histogram_parity(subj, qry, both, edges, labelled, flags):
    import gdist
    e = HIST_EDGES[edges]()
    counts, nans, bad = check_hist(subj, qry, e, flags, labelled=labelled)
    assert counts.shape[0] == (4 if labelled else 1)
    twin = both.histogram(e, Z.LABELS if labelled else None, rows=(NS, NS + NQ), cols=(0, NS), upper=False,
                          method=gdist.METHOD_SORTED, flags=flags)
    assert counts.tobytes() == twin.counts.tobytes() and nans.tobytes() == twin.nans.tobytes()
    if labelled:
        assert bad.tobytes() == twin.bad.tobytes()
        # every series holds the pairs of its group side
        rc, sides, gbad = raw_group(subj, qry, flags=flags)
        assert rc == 0 and np.array_equal(gbad, bad)
        for s, side in enumerate(as_sides(sides)):
            assert counts[s].sum() + nans[s] == side.n + side.ones + side.nans
    if edges == "ulp_inf_one":
        assert counts[:, 0].sum() == 0 and counts[:, -1].sum() == 0       # below -inf, from +inf on
        if not labelled and flags == 0:
            assert counts[0].tolist() == Z.HIST_ULP


# 3 ---- walk cuts -----------------------------------------------------------------
@pytest.mark.parametrize("cols_opt", [None, 64], ids=["cols_default", "cols64"])
@pytest.mark.parametrize("rows_opt", [None, 1, 7], ids=["rows_default", "rows1", "rows7"])
def test_walk_cuts_change_nothing(subj, qry, opts, rows_opt, cols_opt):
    """closest_rows 1 / 7 / default and closest_cols 64 (143 columns in chunks
    of 64 + 64 + 15) / default: every result is the refs'; within does not
    read closest_cols."""
    if rows_opt is not None:
        opts(closest_rows=rows_opt)
    if cols_opt is not None:
        opts(closest_cols=cols_opt)
    check_within(subj, qry, 0.9, EMPTY_NAN)
    check_group(subj, qry, EMPTY_NAN)
    check_hist(subj, qry, Z.EDGES50, EMPTY_NAN)
    check_hist(subj, qry, Z.ulp_edges(), 0, labelled=False)


# 4 ---- sub-rectangles -------------------------------------------------------------
@pytest.mark.parametrize("cols", [(0, 64), (64, 143), (5, 130)])
def test_sub_rectangles(subj, qry, cols):
    rows = (5, 37)
    check_within(subj, qry, 0.9, EMPTY_NAN, rows, cols)
    check_within(subj, qry, 1.0, 0, (40, 52), cols)
    check_group(subj, qry, EMPTY_NAN, (40, 52), cols)
    check_group(subj, qry, 0, rows, cols)
    check_hist(subj, qry, Z.EDGES50, EMPTY_NAN, (40, 52), cols)
    check_hist(subj, qry, Z.ulp_edges(), 0, rows, cols, labelled=False)


def test_disjoint_ranges_combine(subj, qry):
    from gdist import _lib as L
    # within: disjoint row ranges concatenate
    rp, col, d = check_within(subj, qry, 0.9, EMPTY_NAN)
    rp1, col1, d1 = check_within(subj, qry, 0.9, EMPTY_NAN, rows=(0, 23))
    rp2, col2, d2 = check_within(subj, qry, 0.9, EMPTY_NAN, rows=(23, 52))
    assert np.array_equal(np.concatenate([rp1, rp2[1:] + rp1[-1]]), rp)
    assert np.array_equal(np.concatenate([col1, col2]), col)
    assert np.array_equal(bits(np.concatenate([d1, d2])), bits(d))
    # histogram: disjoint column ranges add
    whole = check_hist(subj, qry, Z.EDGES50, EMPTY_NAN)
    a = check_hist(subj, qry, Z.EDGES50, EMPTY_NAN, cols=(0, 64))
    b = check_hist(subj, qry, Z.EDGES50, EMPTY_NAN, cols=(64, 143))
    for w, x, y in zip(whole, a, b):
        assert np.array_equal(x + y, w)
    # group stats: disjoint row ranges merge to the bytes of the whole
    rc, sides, bad = raw_group(subj, qry, flags=EMPTY_NAN)
    rc1, s1, b1 = raw_group(subj, qry, rows=(0, 23), flags=EMPTY_NAN)
    rc2, s2, b2 = raw_group(subj, qry, rows=(23, 52), flags=EMPTY_NAN)
    assert rc == rc1 == rc2 == 0
    assert L.lib.gdist_group_stats_merge(s1.ctypes.data, L.ptr(b1, C.c_int64), s2.ctypes.data,
                                         L.ptr(b2, C.c_int64), Z.NTYPES) == 0
    assert s1.tobytes() == sides.tobytes() and b1.tobytes() == bad.tobytes()


# 5 ---- other collections ------------------------------------------------------------
def _other_labels(n, shift):
    g = np.arange(n, dtype=np.int32) + shift
    lab = (g % 3)[None, :].copy()
    lab[:, g % 5 == 0] = -1
    return np.ascontiguousarray(lab, dtype=np.int32)


def _check_all_from_d(res, qs, D, flags=0):
    """The three calls on any two collections against the refs on their D."""
    ns, nq = len(res), len(qs)
    rc, rowptr, col, d, total = raw_within(res, qs, 0.95, flags=flags)
    erp, ecol, ed = W.within_ref(D, 0.95, upper=False, keep_self=True)
    assert rc == 0 and total == erp[-1] and np.array_equal(rowptr, erp)
    assert np.array_equal(col[:total], ecol) and np.array_equal(bits(d[:total]), bits(ed))
    assert np.all(col[total:] == POISON_COL)
    ql, sl = _other_labels(nq, 1), _other_labels(ns, 0)
    lab = np.concatenate([sl, ql], axis=1)
    rc, sides, bad = raw_group(res, qs, flags=flags, qlab=ql, slab=sl)
    assert rc == 0
    G.check_stats(as_sides(sides), bad, G.group_ref(D, lab, ns, 0, upper=False))
    hc = res.cross_histogram(qs, Z.EDGES50, ql, sl, empty_nan=bool(flags))
    ec, en, eb = H.hist_ref(D, Z.EDGES50, lab, ns, 0, upper=False)
    assert np.array_equal(hc.counts, ec) and np.array_equal(hc.nans, en) and np.array_equal(hc.bad, eb)
    return total


def test_protein_sets(ctx):
    import gdist
    from gdist import synth
    prot = [bytes(r) for r in synth.genomes(20, 700, 0.1, 7, protein=True)]
    s_seqs, q_seqs = prot[:13], prot[13:] + [b"MKV"]
    res = gdist.KmerSets.from_sequences(s_seqs, 8, gdist.KmerType.PROT, 0, ctx)
    qs = gdist.KmerSets.from_sequences(q_seqs, 8, gdist.KmerType.PROT, 0, ctx)
    try:
        off, codes = oracle.pack(s_seqs + q_seqs, 8, 1, 0)
        _, D = oracle.matrix(off, codes, 13, 21, 0, 13, flags=0)
        assert 0 < _check_all_from_d(res, qs, D) < D.size
    finally:
        res.free()
        qs.free()


def test_pack_like_queries(subj):
    s_seqs, q_seqs = X.sequences()
    qs = subj.pack_like(q_seqs[10:25])
    try:
        D = Z.expected_d(0)[10:25]
        assert _check_all_from_d(subj, qs, D) > 0
    finally:
        qs.free()


def test_same_handle_for_both(subj):
    """KEEP_SELF without UPPER: cell (i, i) counts like any other."""
    import gdist
    _, D = subj.matrix(method=gdist.METHOD_SORTED, flags=EMPTY_NAN)
    total = _check_all_from_d(subj, subj, D, flags=EMPTY_NAN)
    rp, cols, d = subj.cross_within(subj, 0.0)
    _, sn = X.sizes()
    own = [int(i) in cols[rp[i]:rp[i + 1]].tolist() for i in range(NS)]
    assert own == (sn > 0).tolist() and total >= int((sn > 0).sum())
    trp, tcols, td = subj.within(0.0, method=gdist.METHOD_SORTED, keep_self=True)
    assert rp.tobytes() == trp.tobytes() and cols.tobytes() == tcols.tobytes() and d.tobytes() == td.tobytes()


# 6 ---- the subjects stay as they are --------------------------------------------------
def test_subjects_untouched(ctx, qry):
    import gdist
    res = gdist.KmerSets.from_sequences(X.sequences()[0], 21, gdist.KmerType.DNA, 0, ctx)
    try:
        res.build_bitsets()
        state = lambda: (res.bitset_info(), res.rare_info(), len(res), res.info())
        before = state()
        off, codes = oracle.pack(X.sequences()[0], 21, 0, 0)
        eI, _ = oracle.matrix(off, codes, 0, NS, 0, NS, flags=0)
        calls = (lambda: check_within(res, qry, 0.9, EMPTY_NAN), lambda: check_group(res, qry, EMPTY_NAN),
                 lambda: check_hist(res, qry, Z.EDGES50, EMPTY_NAN))
        for call in calls:
            call()
            assert state() == before
        aI, _ = res.matrix(method=gdist.METHOD_BITSET)
        assert np.array_equal(aI, eI)
        assert state() == before
    finally:
        res.free()


# 7 ---- refusals ----------------------------------------------------------------------
def test_einval_leaves_outputs_untouched(ctx, subj, qry):
    import gdist
    from gdist import _lib as L
    Null = types.SimpleNamespace(h=None, ctx=ctx)

    def err():
        msg = L.lib.gdist_last_error().decode()
        assert msg
        return msg

    def w(s, q, max_dist=0.9, **kw):
        rc, rowptr, col, d, total = raw_within(s, q, max_dist, **kw)
        assert rc == L.EINVAL and total == POISON_CNT
        assert np.all(rowptr == POISON_RP) and np.all(col == POISON_COL) and np.all(d == POISON_D)
        return err()

    def g(s, q, **kw):
        kw.setdefault("qlab", np.zeros((1, max(len(q), 1) if q.h else 1), np.int32))
        kw.setdefault("slab", np.zeros((1, max(len(s), 1) if s.h else 1), np.int32))
        rc, sides, bad = raw_group(s, q, **kw)
        assert rc == L.EINVAL and np.all(sides == POISON_BYTE) and np.all(bad == POISON_CNT)
        return err()

    def h(s, q, edges=Z.EDGES50, **kw):
        kw.setdefault("labelled", False)
        rc, counts, nans, bad = raw_hist(s, q, edges, **kw)
        assert rc == L.EINVAL
        assert np.all(counts == POISON_CNT) and np.all(nans == POISON_CNT) and np.all(bad == POISON_CNT)
        return err()

    every = lambda *a, **k: (w(*a, **k), g(*a, **k), h(*a, **k))
    # the conditions every cross call shares
    assert all("null sets handle" in t for t in every(subj, Null, rows=(0, 1)))
    assert all("null sets handle" in t for t in every(Null, qry, cols=(0, 1)))
    other = gdist.Context(0)
    foreign = gdist.KmerSets.from_sequences(X.sequences()[1][:3], 21, gdist.KmerType.DNA, 0, other)
    sk = subj.sketches(64)
    k15 = gdist.KmerSets.from_sequences(X.sequences()[1][:3], 15, gdist.KmerType.DNA, 0, ctx)
    fwd = gdist.KmerSets.from_sequences(X.sequences()[1][:3], 21, gdist.KmerType.DNA, 0x1, ctx)
    prot = gdist.KmerSets.from_sequences([b"MKVLAAGIVGLLLAQ"], 8, gdist.KmerType.PROT, 0, ctx)
    bare = gdist.KmerSets.from_sequences(X.sequences()[0][:8], 21, gdist.KmerType.DNA, 0, ctx)
    bare.build_bitsets()
    bare.release_codes()
    try:
        assert all("context" in t for t in every(subj, foreign))
        assert all("context" in t for t in every(foreign, qry))
        assert all("context" in t for t in every(subj, qry, ctx=other))
        assert all("kmer sets" in t for t in every(sk, qry, cols=(0, 10)))
        assert all("kmer sets" in t for t in every(subj, sk, rows=(0, 10)))
        for odd in (k15, fwd, prot):
            assert all("different kmer specs" in t for t in every(subj, odd, rows=(0, 1)))
            assert all("different kmer specs" in t for t in every(odd, qry, cols=(0, 1)))
        assert all("no codes" in t for t in every(bare, qry))
        assert all("no codes" in t for t in every(subj, bare))
    finally:
        for x in (foreign, sk, k15, fwd, prot, bare):
            x.free()
        other.close()
    for rows in ((-1, 5), (5, 4), (0, NQ + 1)):
        assert all("query range" in t for t in every(subj, qry, rows=rows))
    for cols in ((-1, 5), (5, 4), (0, NS + 1)):
        assert all("column range" in t for t in every(subj, qry, cols=cols))
    for flags in (UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF, 0x800, EMPTY_NAN | UPPER_TRIANGLE):
        assert all("GDIST_EMPTY_NAN" in t for t in every(subj, qry, flags=flags))
    # within's own
    assert "NaN" in w(subj, qry, max_dist=float("nan"))
    assert "capacity" in w(subj, qry, capacity=-1)
    assert "rowptr_out" in w(subj, qry, null_rowptr=True)
    assert "total" in w(subj, qry, null_total=True)
    assert "col_out" in w(subj, qry, capacity=5, null_lists=True)
    # group stats' own
    assert "ntypes" in g(subj, qry, ntypes=0)
    assert "ntypes" in g(subj, qry, ntypes=9)
    for name in ("qlabels", "slabels", "out", "bad"):
        assert "null" in g(subj, qry, null=(name,))
    # histogram's own
    assert "nedges" in h(subj, qry, nedges=0)
    assert "nedges" in h(subj, qry, edges=np.arange(1024.0))
    assert "ntypes" in h(subj, qry, ntypes=-1)
    assert "ntypes" in h(subj, qry, labelled=True, ntypes=9)
    assert "ascending" in h(subj, qry, edges=[0.5, 0.5])
    assert "ascending" in h(subj, qry, edges=[0.5, 0.25])
    assert "ascending" in h(subj, qry, edges=[-0.0, 0.0])
    assert "NaN" in h(subj, qry, edges=[0.5, float("nan")])
    for name in ("edges", "counts", "nans"):
        assert "null" in h(subj, qry, null=(name,))
    for name in ("qlabels", "slabels", "bad"):
        assert "null" in h(subj, qry, labelled=True, null=(name,))


def test_empty_ranges_are_ok(subj, qry):
    from gdist.kmers import GroupStats
    for rows, cols in (((4, 4), None), (None, (9, 9)), ((0, 0), (0, 0))):
        nr = (rows[1] - rows[0]) if rows else NQ
        rc, rowptr, col, d, total = raw_within(subj, qry, 0.9, rows, cols, capacity=6)
        assert rc == 0 and total == 0 and rowptr.tolist() == [0] * (nr + 1)
        assert np.all(col == POISON_COL) and np.all(d == POISON_D)
        rc, sides, bad = raw_group(subj, qry, rows, cols)
        assert rc == 0 and np.all(bad == 0)
        for s in as_sides(sides):
            assert (s.n, s.ones, s.nans) == (0, 0, 0) and (s.min, s.max, s.mean, s.sdev) == (1.0, 1.0, 1.0, 0.0)
            assert list(s.sum) == [0, 0] and list(s.sumsq) == [0, 0, 0]
        assert sides.tobytes() + bad.tobytes() == GroupStats.empty(Z.NTYPES).tobytes()
        for labelled in (False, True):
            rc, counts, nans, bad = raw_hist(subj, qry, Z.EDGES50, rows, cols, labelled=labelled)
            assert rc == 0 and not counts.any() and not nans.any()
            assert np.all(bad == (0 if labelled else POISON_CNT))


# 8 ---- the genomes table over a resident base collection ----------------------------------
def _genomes(seqs, prefix):
    from gdist.processors import Genome
    return [Genome(f"{prefix}{i}.1", f"{prefix} genome {i}", [s.decode()]) for i, s in enumerate(seqs)]


@pytest.mark.parametrize("within", [False, True], ids=["every_pair", "within"])
def test_genomes_against_text(ctx, within):
    import gdist
    from gdist.processors import genome_distance, genomes_against
    s_seqs, q_seqs = X.sequences()
    base = _genomes(s_seqs[:5] + [s_seqs[77], s_seqs[NS - 1]], "B")        # two duplicated subjects, the empty one
    comps = _genomes(q_seqs[:3] + q_seqs[-2:], "C")
    want = io.StringIO()
    n_want = genome_distance(base, [comps[:2], comps[2:]], want, 21, 0.9, ctx=ctx, within=within)
    db = gdist.KmerSets.from_sequences([g.kmer_text() for g in base], 21, gdist.KmerType.DNA, 0, ctx)
    try:
        for batch in (64, 2):
            out = io.StringIO()
            assert genomes_against(db, base, iter(comps), out, 0.9, within=within, batch=batch) == n_want
            assert out.getvalue() == want.getvalue()
        assert len(db) == len(base)
    finally:
        db.free()
    lines = want.getvalue().splitlines()
    assert lines[0] == "genome1\tgenome2\tdistance"
    assert (1 < len(lines) < 1 + 5 * 7) if within else len(lines) == 1 + 5 * 7


# 9 ---- gdist_ctx_cross_info ------------------------------------------------------------------
def test_cross_info_reports_these_calls(ctx, subj, qry, opts):
    check_within(subj, qry, 0.9)
    join_ms, select_ms, units = ctx.cross_info()
    assert (join_ms, select_ms) == (-1.0, -1.0) and units > 0      # option time_kernels is off
    check_group(subj, qry)
    assert ctx.cross_info()[2] > 0
    opts(time_kernels=1)
    for call in (lambda: check_within(subj, qry, 0.9), lambda: check_group(subj, qry),
                 lambda: check_hist(subj, qry, Z.EDGES50)):
        call()
        join_ms, select_ms, n = ctx.cross_info()
        assert join_ms >= 0 and select_ms >= 0 and n > 0
