"""New query sets against a resident collection on the device
(gdist_cross_matrix / gdist_cross_closest; FindProcessor.java:94-110 keeps its
database loaded and answers one getClosest per genome). Every answer is
compared bit for bit: I with array_equal, D and the neighbour distances through
their uint64 views, against the oracle's matrix sliced to queries x subjects
(cross_ref.py) or a full sort of it (closest_ref). Outputs are pre-filled with
poison, so a cell the call leaves unwritten, or writes outside its rectangle,
fails. Not covered: a subject collection of 2^32 - 1 sets (it does not fit a
test)."""
import ctypes as C
import io
import types

import numpy as np
import pytest

import closest_ref as R
import cross_ref as X
import oracle

pytestmark = pytest.mark.gpu

EMPTY_NAN, UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF = 0x400, 0x100, 0x200, 0x1000
POISON_I, POISON_D, POISON_IDX, POISON_CNT = -77, 7.5, 0x5A5A5A5A5A5A5A5A, -9


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def raw_matrix(subj, qry, rows=None, cols=None, flags=0, pad=0, want_I=True, want_D=True, ctx=None):
    """gdist_cross_matrix into poisoned host arrays of row stride nc + pad:
    (rc, I[nr, ld] | None, D[nr, ld] | None)."""
    from gdist import _lib as L
    r0, r1 = rows or (0, len(qry))
    c0, c1 = cols or (0, len(subj))
    nr, nc = max(r1 - r0, 0), max(c1 - c0, 0)
    ld = nc + pad
    I = np.full((max(nr, 1), max(ld, 1)), POISON_I, dtype=np.int32)
    D = np.full((max(nr, 1), max(ld, 1)), POISON_D, dtype=np.float64)
    rc = L.lib.gdist_cross_matrix((ctx or subj.ctx).h, qry.h, subj.h, r0, r1, c0, c1, flags,
                                  L.ptr(I, C.c_int32) if want_I else None,
                                  L.ptr(D, C.c_double) if want_D else None, max(ld, 1))
    return rc, I, D


def raw_closest(subj, qry, n, max_dist, rows=None, cols=None, flags=0):
    """gdist_cross_closest into poisoned outputs: (rc, idx[nr, n], d[nr, n], count[nr])."""
    from gdist import _lib as L
    r0, r1 = rows or (0, len(qry))
    nr, m = max(r1 - r0, 0), max(n, 0)
    c0, c1 = cols or (0, len(subj))
    idx = np.full(max(nr * m, 1), POISON_IDX, dtype=np.int64)
    d = np.full(max(nr * m, 1), POISON_D, dtype=np.float64)
    cnt = np.full(max(nr, 1), POISON_CNT, dtype=np.int32)
    rc = L.lib.gdist_cross_closest(subj.ctx.h, qry.h, subj.h, r0, r1, c0, c1, flags, n, max_dist,
                                   L.ptr(idx, C.c_int64), L.ptr(d, C.c_double), L.ptr(cnt, C.c_int32))
    return rc, idx[:nr * m].reshape(nr, m), d[:nr * m].reshape(nr, m), cnt[:nr]


def oracle_cross(subj_seqs, qry_seqs, k=21, kind=0, pack_flags=0, flags=0):
    """(I, D) [queries, subjects] of the oracle over the packed concatenation."""
    ns, nq = len(subj_seqs), len(qry_seqs)
    off, codes = oracle.pack(list(subj_seqs) + list(qry_seqs), k, kind, pack_flags)
    return oracle.matrix(off, codes, ns, ns + nq, 0, ns, flags=flags)


def check_matrix(subj, qry, eI, eD, rows=None, cols=None, flags=0):
    rc, I, D = raw_matrix(subj, qry, rows, cols, flags)
    assert rc == 0
    assert np.array_equal(I, eI)
    assert np.array_equal(bits(D), bits(eD))


@pytest.fixture(scope="module")
def subj(ctx):
    import gdist
    X.check_fixture()
    s = gdist.KmerSets.from_sequences(X.sequences()[0], 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


@pytest.fixture(scope="module")
def qry(ctx):
    import gdist
    s = gdist.KmerSets.from_sequences(X.sequences()[1], 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


# 1 ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["plain", "empty_nan"])
def test_full_fixture_parity(ctx, subj, qry, flags):
    """The whole 52 x 143 rectangle; its (row, block)s are cut by segment
    range, so the units' atomic adds ran."""
    eI, eD = X.expected(flags)
    check_matrix(subj, qry, eI, eD, flags=flags)
    join_ms, select_ms, units = ctx.cross_info()
    qn, _ = X.sizes()
    blocks = -(-X.NS // 64)
    assert units > int((qn > 0).sum()) * blocks
    assert (join_ms, select_ms) == (-1.0, -1.0)          # option time_kernels is off


def test_cross_info_times(ctx, subj, qry, opts):
    opts(time_kernels=1)
    eI, eD = X.expected(0)
    check_matrix(subj, qry, eI, eD)
    join_ms, select_ms, units = ctx.cross_info()
    assert join_ms > 0 and select_ms > 0 and units > 0
    rc, idx, d, cnt = raw_closest(subj, qry, 10, 0.9)
    assert rc == 0
    join_ms, select_ms, units = ctx.cross_info()
    assert join_ms > 0 and select_ms > 0 and units > 0


# 2 ---------------------------------------------------------------------------
@pytest.mark.parametrize("want", ["both", "I", "D"])
def test_sub_rectangle_and_padding(subj, qry, want):
    """Rows (5, 37) x cols (60, 143): the blocks start at 60, 124 and 188 is
    past the end, so they straddle the collection's multiples of 64. The row
    stride is nc + 3: the padding and a null output's array keep the poison."""
    rows, cols = (5, 37), (60, 143)
    nc = cols[1] - cols[0]
    eI, eD = X.expected(0)
    rc, I, D = raw_matrix(subj, qry, rows, cols, 0, pad=3, want_I=want != "D", want_D=want != "I")
    assert rc == 0
    assert np.all(I[:, nc:] == POISON_I) and np.all(D[:, nc:] == POISON_D)
    if want != "D":
        assert np.array_equal(I[:, :nc], eI[5:37, 60:143])
    else:
        assert np.all(I == POISON_I)
    if want != "I":
        assert np.array_equal(bits(D[:, :nc]), bits(eD[5:37, 60:143]))
    else:
        assert np.all(D == POISON_D)


@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["plain", "empty_nan"])
def test_matrix_walk_cuts(subj, qry, opts, flags):
    """closest_rows 4 x closest_cols 4 over rows (1, 10) x cols (0, 10): row
    blocks of 4, 4 and 1 rows against column chunks of 4, 4 and 2 columns, nine
    steps. The arrays, padding included, are the bytes of the one-step call and
    the cells are the oracle's."""
    rows, cols = (1, 10), (0, 10)
    eI, eD = X.expected(flags)
    rc, I1, D1 = raw_matrix(subj, qry, rows, cols, flags, pad=3)
    assert rc == 0
    opts(closest_rows=4, closest_cols=4)
    rc, I, D = raw_matrix(subj, qry, rows, cols, flags, pad=3)
    assert rc == 0
    assert I.tobytes() == I1.tobytes() and D.tobytes() == D1.tobytes()
    assert np.all(I[:, 10:] == POISON_I) and np.all(D[:, 10:] == POISON_D)
    assert np.array_equal(I[:, :10], eI[1:10, 0:10])
    assert np.array_equal(bits(D[:, :10]), bits(eD[1:10, 0:10]))


# 3 ---------------------------------------------------------------------------
def test_same_handle_for_both(subj):
    import gdist
    mI, mD = subj.matrix(method=gdist.METHOD_SORTED)
    check_matrix(subj, subj, mI, mD)
    # every set is its own nearest neighbour: nothing is left out as self
    rc, idx, d, cnt = raw_closest(subj, subj, 1, 0.0)
    assert rc == 0
    _, sn = X.sizes()
    assert np.array_equal(cnt, (sn > 0).astype(np.int32))
    assert np.all(idx[sn > 0, 0] <= np.flatnonzero(sn > 0))


# 4 ---------------------------------------------------------------------------
def test_resident_collection_untouched(ctx, qry):
    import gdist
    res = gdist.KmerSets.from_sequences(X.sequences()[0], 21, gdist.KmerType.DNA, 0, ctx)
    try:
        res.build_bitsets()
        state = lambda: (res.bitset_info(), res.rare_info(), res.sparse_info(), res.build_timing(), len(res),
                         res.info())
        before = state()
        bI, bD = res.matrix(method=gdist.METHOD_BITSET)
        eI, eD = X.expected(0)
        check_matrix(res, qry, eI, eD)
        rc, idx, d, cnt = raw_closest(res, qry, 10, 0.9)
        assert rc == 0
        assert state() == before
        aI, aD = res.matrix(method=gdist.METHOD_BITSET)
        assert np.array_equal(aI, bI) and np.array_equal(bits(aD), bits(bD))
        assert res.prepare(gdist.METHOD_AUTO)[0] == gdist.METHOD_BITSET
        assert state() == before
    finally:
        res.free()


# 5 ---------------------------------------------------------------------------
def test_appends(ctx):
    import gdist
    s_seqs, q_seqs = X.sequences()
    s0, s_add = s_seqs[40:110], s_seqs[0:9] + [b"", s_seqs[130]]
    q0, q_add = q_seqs[20:40], [q_seqs[0], b"ACGT", q_seqs[45]]
    res = gdist.KmerSets.from_sequences(s0, 21, gdist.KmerType.DNA, 0, ctx)
    qs = gdist.KmerSets.from_sequences(q0, 21, gdist.KmerType.DNA, 0, ctx)
    try:
        eI, eD = oracle_cross(s0, q0)
        check_matrix(res, qs, eI, eD)                      # builds the subjects' segment index
        assert res.append(s_add) == len(s0)                # ... which the append extends
        eI, eD = oracle_cross(s0 + s_add, q0)
        assert eI.shape == (20, 81)
        check_matrix(res, qs, eI, eD)
        assert qs.append(q_add) == len(q0)
        eI, eD = oracle_cross(s0 + s_add, q0 + q_add, flags=EMPTY_NAN)
        assert int(np.isnan(eD).sum()) == 1 and eI.shape == (23, 81)   # b"ACGT" x b""
        check_matrix(res, qs, eI, eD, flags=EMPTY_NAN)
        rc, idx, d, cnt = raw_closest(res, qs, 5, 0.95)
        assert rc == 0
        xi, xd, xc = R.closest_ref(eD, 5, 0.95, keep_self=True)
        assert np.array_equal(cnt, xc) and np.array_equal(idx, xi) and np.array_equal(bits(d), bits(xd))
    finally:
        res.free()
        qs.free()


# 6 ---------------------------------------------------------------------------
def test_protein_one_segment(ctx):
    """Protein k = 8 sets under 2,048 codes: one segment, one unit a (row, block)."""
    import gdist
    from gdist import synth
    prot = [bytes(r) for r in synth.genomes(90, 700, 0.1, 7, protein=True)]
    s_seqs, q_seqs = prot[:70], prot[70:] + [b"MKV"]
    res = gdist.KmerSets.from_sequences(s_seqs, 8, gdist.KmerType.PROT, 0, ctx)
    qs = gdist.KmerSets.from_sequences(q_seqs, 8, gdist.KmerType.PROT, 0, ctx)
    try:
        assert int(max(res.sizes().max(), qs.sizes().max())) < 2048
        eI, eD = oracle_cross(s_seqs, q_seqs, k=8, kind=1)
        assert int((eI > 0).sum()) > 1000
        check_matrix(res, qs, eI, eD)
        assert ctx.cross_info()[2] == 20 * 2               # 20 non-empty rows x 2 blocks
    finally:
        res.free()
        qs.free()


def test_long_query_segment_in_sub_chunks(ctx):
    """Short subjects (one segment) and a 3,000 bp query: 5,960 keys in one
    segment, more than one fill of the 4,096-key table."""
    import gdist
    from gdist import synth
    g = bytes(synth.genomes(1, 3000, 0.0, 55)[0])
    s_seqs = [g[i * 35:i * 35 + 500] for i in range(70)] + [bytes(synth.genomes(1, 500, 0.0, 56)[0])]
    q_seqs = [g, g[100:900]]
    res = gdist.KmerSets.from_sequences(s_seqs, 21, gdist.KmerType.DNA, 0, ctx)
    qs = gdist.KmerSets.from_sequences(q_seqs, 21, gdist.KmerType.DNA, 0, ctx)
    try:
        assert int(res.sizes().max()) <= 2048 and int(qs.sizes()[0]) == 5960
        eI, eD = oracle_cross(s_seqs, q_seqs)
        assert int(eI[0, :70].min()) == 960 and eI[0, 70] == 0
        check_matrix(res, qs, eI, eD)
        assert ctx.cross_info()[2] == 2 * 2                # nseg = 1: no cut
    finally:
        res.free()
        qs.free()


def test_all_ones_code(ctx):
    """DNA k = 32, forward strand: T x 32 is the all-ones code, the hash
    table's empty marker, in a query and in a subject."""
    import gdist
    from gdist import synth
    fwd = 0x1
    rnd = [bytes(r) for r in synth.genomes(3, 200, 0.05, 9)]
    s_seqs = [b"T" * 33 + b"ACGT", rnd[0], b"T" * 31, rnd[1] + b"T" * 32]
    q_seqs = [b"T" * 40, rnd[2], rnd[0] + b"T" * 35, b""]
    res = gdist.KmerSets.from_sequences(s_seqs, 32, gdist.KmerType.DNA, fwd, ctx)
    qs = gdist.KmerSets.from_sequences(q_seqs, 32, gdist.KmerType.DNA, fwd, ctx)
    try:
        off, codes = qs.download()
        assert off[1] == 1 and codes[0] == np.uint64(0xFFFFFFFFFFFFFFFF)
        eI, eD = oracle_cross(s_seqs, q_seqs, k=32, pack_flags=fwd, flags=EMPTY_NAN)
        assert eI[0].tolist() == [1, 0, 0, 1] and eI[2, 0] == 1 and eI[2, 1] == 169
        assert np.isnan(eD[3, 2]) and int(np.isnan(eD).sum()) == 1
        check_matrix(res, qs, eI, eD, flags=EMPTY_NAN)
    finally:
        res.free()
        qs.free()


def test_empty_query_alone_and_one_subject(ctx, subj, qry):
    qn, _ = X.sizes()
    assert qn[51] == 0
    for flags in (0, EMPTY_NAN):
        eI, eD = X.expected(flags)
        check_matrix(subj, qry, eI[51:52], eD[51:52], rows=(51, 52), flags=flags)
        assert ctx.cross_info()[2] == 0                    # an empty set gets no unit
        check_matrix(subj, qry, eI[:, 5:6], eD[:, 5:6], cols=(5, 6), flags=flags)
        check_matrix(subj, qry, eI[:, 142:143], eD[:, 142:143], cols=(142, 143), flags=flags)
        check_matrix(subj, qry, eI[7:8, 77:78], eD[7:8, 77:78], rows=(7, 8), cols=(77, 78), flags=flags)


# 7 ---------------------------------------------------------------------------
CLOSEST = [(10, 0.9), (1, 0.9), (10, 1.0), (200, 1.0), (10, 0.0), (0, 0.9)]


def check_closest(subj, qry, n, max_dist, flags, rows=None, cols=None):
    D = X.expected(flags)[1]
    r0, r1 = rows or (0, X.NQ)
    c0, c1 = cols or (0, X.NS)
    rc, idx, d, cnt = raw_closest(subj, qry, n, max_dist, rows, cols, flags)
    assert rc == 0
    eidx, ed, ecnt = R.closest_ref(D[r0:r1, c0:c1], n, max_dist, r0, c0, keep_self=True)
    assert np.array_equal(cnt, ecnt)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(bits(d), bits(ed))
    return eidx, ed, ecnt


@pytest.mark.parametrize("blocks", ["default", "rows7_cols50"])
@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["plain", "empty_nan"])
@pytest.mark.parametrize("n,max_dist", CLOSEST)
def test_closest_against_reference(subj, qry, opts, n, max_dist, flags, blocks):
    if blocks != "default":
        opts(closest_rows=7, closest_cols=50)
    check_closest(subj, qry, n, max_dist, flags)


@pytest.mark.parametrize("blocks", ["default", "rows7_cols50"])
def test_closest_sub_ranges(subj, qry, opts, blocks):
    if blocks != "default":
        opts(closest_rows=7, closest_cols=50)
    check_closest(subj, qry, 10, 0.9, 0, cols=(60, 143))
    check_closest(subj, qry, 10, 1.0, EMPTY_NAN, rows=(5, 52), cols=(100, 143))
    check_closest(subj, qry, 3, 1.0, 0, rows=(51, 52))


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("n,max_dist,flags", [(10, 0.9, 0), (10, 1.0, EMPTY_NAN), (200, 1.0, 0)])
def test_closest_against_concat_route(subj, qry, n, max_dist, flags):
    """The same answer the way it was reached before: gdist_closest over
    subjects.concat(queries), rows [143, 195) x cols [0, 143)."""
    import gdist
    both = subj.concat(qry)
    try:
        assert len(both) == X.NS + X.NQ
        eidx, ed, ecnt = both.closest(n, max_dist, rows=(X.NS, X.NS + X.NQ), cols=(0, X.NS),
                                      method=gdist.METHOD_SORTED, flags=flags)
        mI, mD = both.matrix(rows=(X.NS, X.NS + X.NQ), cols=(0, X.NS), method=gdist.METHOD_SORTED, flags=flags)
    finally:
        both.free()
    rc, idx, d, cnt = raw_closest(subj, qry, n, max_dist, flags=flags)
    assert rc == 0
    assert np.array_equal(cnt, ecnt) and np.array_equal(idx, eidx) and np.array_equal(bits(d), bits(ed))
    check_matrix(subj, qry, mI, mD, flags=flags)


# 9 ---------------------------------------------------------------------------
def _refused(rc, *arrays):
    from gdist import _lib as L
    assert rc == L.EINVAL
    for a, poison in arrays:
        assert np.all(a == poison)


def test_einval_leaves_outputs_untouched(ctx, subj, qry):
    import gdist
    from gdist import _lib as L

    Null = types.SimpleNamespace(h=None, ctx=ctx)

    def m(s, q, rows=None, cols=None, flags=0, pad=0, want_I=True, want_D=True, c=None):
        rc, I, D = raw_matrix(s, q, rows, cols, flags, pad, want_I, want_D, ctx=c)
        _refused(rc, (I, POISON_I), (D, POISON_D))
        return L.lib.gdist_last_error().decode()

    def c(s, q, n=3, max_dist=0.9, rows=None, cols=None, flags=0):
        rc, idx, d, cnt = raw_closest(s, q, n, max_dist, rows, cols, flags)
        _refused(rc, (idx, POISON_IDX), (d, POISON_D), (cnt, POISON_CNT))
        return L.lib.gdist_last_error().decode()

    both = lambda *a, **k: (m(*a, **k), c(*a, **k))
    # null handles
    assert "null sets handle" in m(subj, Null, rows=(0, 1))
    assert "null sets handle" in m(Null, qry, cols=(0, 1))
    assert "null sets handle" in c(subj, Null, rows=(0, 1))
    assert "null sets handle" in c(Null, qry, cols=(0, 1))
    # another context
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
        assert all("context" in t for t in both(subj, foreign))
        assert all("context" in t for t in both(foreign, qry))
        assert "context" in m(subj, qry, c=other)
        assert all("kmer sets" in t for t in both(sk, qry, cols=(0, 10)))
        assert all("kmer sets" in t for t in both(subj, sk, rows=(0, 10)))
        for odd in (k15, fwd, prot):
            assert all("different kmer specs" in t for t in both(subj, odd, rows=(0, 1)))
            assert all("different kmer specs" in t for t in both(odd, qry, cols=(0, 1)))
        assert all("no codes" in t for t in both(bare, qry))
        assert all("no codes" in t for t in both(subj, bare))
    finally:
        for h in (foreign, sk, k15, fwd, prot, bare):
            h.free()
        other.close()
    # ranges
    for rows in ((-1, 5), (5, 4), (0, X.NQ + 1)):
        assert all("query range" in t for t in both(subj, qry, rows=rows))
    for cols in ((-1, 5), (5, 4), (0, X.NS + 1)):
        assert all("column range" in t for t in both(subj, qry, cols=cols))
    assert "leading dimension" in m(subj, qry, pad=-1)
    assert "both outputs null" in m(subj, qry, want_I=False, want_D=False)
    for flags in (UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF, 0x800, EMPTY_NAN | UPPER_TRIANGLE):
        assert all("GDIST_EMPTY_NAN" in t for t in both(subj, qry, flags=flags))
    assert "GDIST_CLOSEST_MAX_N" in c(subj, qry, n=-1)
    assert "GDIST_CLOSEST_MAX_N" in c(subj, qry, n=513)
    assert "NaN" in c(subj, qry, max_dist=float("nan"))
    d = np.full(8, POISON_D)
    cnt = np.full(8, POISON_CNT, dtype=np.int32)
    idx = np.full(8, POISON_IDX, dtype=np.int64)
    args = (ctx.h, qry.h, subj.h, 0, 2, 0, X.NS, 0, 2, 0.9)
    assert L.lib.gdist_cross_closest(*args, None, L.ptr(d, C.c_double), L.ptr(cnt, C.c_int32)) == L.EINVAL
    assert L.lib.gdist_cross_closest(*args, L.ptr(idx, C.c_int64), None, L.ptr(cnt, C.c_int32)) == L.EINVAL
    assert L.lib.gdist_cross_closest(*args, L.ptr(idx, C.c_int64), L.ptr(d, C.c_double), None) == L.EINVAL
    assert "null output" in L.lib.gdist_last_error().decode()
    assert np.all(d == POISON_D) and np.all(cnt == POISON_CNT) and np.all(idx == POISON_IDX)


def test_empty_ranges_are_ok(subj, qry):
    from gdist import _lib as L
    for rows, cols in (((4, 4), None), (None, (9, 9)), ((0, 0), (0, 0))):
        rc, I, D = raw_matrix(subj, qry, rows, cols)
        assert rc == 0 and np.all(I == POISON_I) and np.all(D == POISON_D)
    # both outputs null is fine when there is nothing to write
    assert raw_matrix(subj, qry, (4, 4), None, want_I=False, want_D=False)[0] == 0
    rc, idx, d, cnt = raw_closest(subj, qry, 4, 0.9, rows=(4, 4))
    assert rc == 0 and idx.size == 0 and cnt.size == 0
    rc, idx, d, cnt = raw_closest(subj, qry, 4, 0.9, cols=(9, 9))
    assert rc == 0 and np.all(cnt == 0) and np.all(idx == -1) and np.all(d == 1.0)
    assert idx.shape == (X.NQ, 4)
    # no output is needed for an empty row range
    assert L.lib.gdist_cross_closest(subj.ctx.h, qry.h, subj.h, 3, 3, 0, X.NS, 0, 4, 0.9, None, None, None) == 0


# 10 --------------------------------------------------------------------------
def _genomes(seqs, prefix):
    from gdist.processors import Genome
    return [Genome(f"{prefix}{i}.1", f"{prefix} genome {i}", [s.decode()]) for i, s in enumerate(seqs)]


@pytest.mark.parametrize("neighbors,max_dist", [(10, 0.9), (10, 1.0), (3, 0.0)])
def test_find_genomes_text(subj, neighbors, max_dist):
    from gdist.javafmt import java_format_f
    from gdist.processors import find_genomes
    s_seqs, q_seqs = X.sequences()
    subjects, queries = _genomes(s_seqs, "S"), _genomes(q_seqs, "Q")
    eidx, ed, ecnt = R.closest_ref(X.expected(0)[1], neighbors, max_dist, keep_self=True)
    lines = ["genome_id\tgenome_name\tneighbor_id\tneighbor_name\tdistance\n"]
    for a, q in enumerate(queries):
        for r in range(ecnt[a]):
            s = subjects[int(eidx[a, r])]
            lines.append(f"{q.id}\t{q.name}\t{s.id}\t{s.name}\t{java_format_f(float(ed[a, r]), 8, 3)}\n")
    want = "".join(lines)
    assert "   0.000\n" in want                        # the duplicates come first
    n_before = len(subj)
    out = io.StringIO()
    found, fail = find_genomes(subj, subjects, queries, out, neighbors, max_dist)
    assert out.getvalue() == want
    assert (found, fail) == (int(ecnt.sum()), int((ecnt == 0).sum()))
    out20 = io.StringIO()
    assert find_genomes(subj, subjects, iter(queries), out20, neighbors, max_dist, batch=20) == (found, fail)
    assert out20.getvalue() == want
    assert len(subj) == n_before
