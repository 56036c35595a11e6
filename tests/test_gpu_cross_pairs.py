"""A pair list across two collections in one device call (gdist_cross_pairs;
MethodTableProcessor.java:258-276 walks such an (id1, id2) list): rows index
the queries, columns the resident subjects. Every answer is compared with `==`
(I, and the fp64 bits of D) against the oracle's cells (cross_pairs_ref), and
against the library's other routes to the same cells. The outputs are
pre-filled with garbage plus 3 guard slots past the list, so a slot the call
leaves unwritten fails and a guard slot it touches fails too. Each property of
a fixture a test relies on is asserted on the oracle's side first
(test_cross_pairs_host.py)."""
import ctypes as C
import types

import numpy as np
import pytest

import closest_ref as CR
import cross_pairs_ref as P
import cross_ref as X
import oracle
import pairs_ref

pytestmark = pytest.mark.gpu

NS, NQ = P.NS, P.NQ
EMPTY_NAN, UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF, SKETCH_JACCARD = 0x400, 0x100, 0x200, 0x1000, 0x800
SORTED, BITSET, AUTO = 1, 2, 0
GARBAGE_I, GARBAGE_D = 0x5A5A5A5A, 7.5


def raw(qry, subj, rows, cols, flags=0, null=(), npairs=None, ctx=None):
    """gdist_cross_pairs into garbage-filled outputs with 3 guard slots: (rc, I, D).
    `null`: the arguments handed over as NULL (of "rows", "cols", "I", "D")."""
    from gdist import _lib as L
    rows = np.ascontiguousarray(rows, np.int64)
    cols = np.ascontiguousarray(cols, np.int64)
    n = len(rows) if npairs is None else npairs
    I = np.full(len(rows) + 3, GARBAGE_I, dtype=np.int32)
    D = np.full(len(rows) + 3, GARBAGE_D, dtype=np.float64)
    rb = rows if len(rows) else np.zeros(1, np.int64)
    cb = cols if len(cols) else np.zeros(1, np.int64)
    rc = L.lib.gdist_cross_pairs((ctx or subj.ctx).h, qry.h, subj.h, n,
                                 None if "rows" in null else L.ptr(rb, C.c_int64),
                                 None if "cols" in null else L.ptr(cb, C.c_int64), flags,
                                 None if "I" in null else L.ptr(I, C.c_int32),
                                 None if "D" in null else L.ptr(D, C.c_double))
    return rc, I, D


def untouched(I, D):
    return bool(np.all(I == GARBAGE_I) and np.all(D == GARBAGE_D))


def last_error():
    from gdist import _lib as L
    return L.lib.gdist_last_error().decode()


def answer(qry, subj, rows, cols, flags=0, null=()):
    """The call's (I, D) cut to the list; the guard slots and a null output's array keep the garbage."""
    rc, I, D = raw(qry, subj, rows, cols, flags, null)
    assert rc == 0, last_error()
    n = len(rows)
    assert np.all(I[n:] == GARBAGE_I) and np.all(D[n:] == GARBAGE_D)
    if "I" in null:
        assert np.all(I == GARBAGE_I)
    if "D" in null:
        assert np.all(D == GARBAGE_D)
    return I[:n], D[:n]


def check(qry, subj, xI, xD, rows, cols, flags=0, null=()):
    I, D = answer(qry, subj, rows, cols, flags, null)
    if "I" not in null:
        bad = np.flatnonzero(I != xI)
        assert len(bad) == 0, (bad[:5], I[bad[:5]], xI[bad[:5]])
    if "D" not in null:
        assert np.array_equal(D.view(np.uint64), np.ascontiguousarray(xD).view(np.uint64))
    return I, D


def same_bytes(a, b):
    return all(np.array_equal(np.ascontiguousarray(x).view(np.uint8), np.ascontiguousarray(y).view(np.uint8))
               for x, y in zip(a, b))


def chunks_of(rows):
    counts = np.unique(rows, return_counts=True)[1]
    return len(counts), int(((counts + 63) // 64).sum())


@pytest.fixture(scope="module")
def subj(ctx):
    import gdist
    P.check_fixture()
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
@pytest.mark.parametrize("name", ["singletons", "long_group", "unit_edges", "mixed"])
def test_lists(subj, qry, name):
    """The four list shapes; pairs_info's groups are the list's distinct rows,
    its units at least one per 64 pairs of a row, and strictly more for the
    long group: its chunks are cut by segment range."""
    rows, cols = P.lists()[name]
    check(qry, subj, *P.pairs_ref(0, rows, cols), rows, cols)
    ms, groups, units = qry.pairs_info()
    ngroups, chunks = chunks_of(rows)
    assert groups == ngroups and ms == -1.0
    assert units >= chunks
    if name == "long_group":
        assert units > chunks, (units, chunks)
    if name == "mixed":
        I, D = check(qry, subj, *P.pairs_ref(EMPTY_NAN, rows, cols), rows, cols, EMPTY_NAN)
        assert int(np.isnan(D).sum()) == int(((rows == P.EMPTY_Q) & (cols == P.KMERLESS_S)).sum()) > 0


def test_outputs_and_timing(subj, qry, opts):
    rows, cols = P.lists()["unit_edges"]
    xI, xD = P.pairs_ref(0, rows, cols)
    check(qry, subj, xI, xD, rows, cols, null=("I",))
    check(qry, subj, xI, xD, rows, cols, null=("D",))
    opts(time_kernels=1)
    check(qry, subj, xI, xD, rows, cols)
    assert qry.pairs_info()[0] >= 0.0
    opts(time_kernels=0)
    check(qry, subj, xI, xD, rows, cols)
    assert qry.pairs_info()[0] == -1.0


# 2 ---------------------------------------------------------------------------
def test_order_independence(subj, qry):
    rows, cols = P.lists()["mixed"]
    xI, xD = P.pairs_ref(0, rows, cols)
    base = check(qry, subj, xI, xD, rows, cols)
    assert same_bytes(base, answer(qry, subj, rows, cols))                     # two runs
    p = np.random.default_rng(5).permutation(len(rows))
    assert same_bytes((base[0][p], base[1][p]), answer(qry, subj, rows[p], cols[p]))
    rev = answer(qry, subj, rows[::-1], cols[::-1])
    assert same_bytes((base[0][::-1], base[1][::-1]), rev)
    # a pair's slot does not depend on the rest of the list
    assert same_bytes((base[0][:37], base[1][:37]), answer(qry, subj, rows[:37], cols[:37]))


# 3 ---------------------------------------------------------------------------
def test_same_handle_for_both(ctx):
    """One collection passed twice: the bytes of gdist_pairs(SORTED), for a
    list with i == j and the two empty sets (no self rule: the join counts |A_i|)."""
    import gdist
    R = pairs_ref
    seqs, off, _, _ = CR.recipe()
    assert np.diff(off)[[R.EMPTY_A, R.EMPTY_B]].tolist() == [0, 0]
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    try:
        rows, cols = R.recipe_lists()["mixed"]
        pairs = list(zip(rows.tolist(), cols.tolist()))
        for p in ((R.NONEMPTY, R.NONEMPTY), (R.EMPTY_A, R.EMPTY_A), (R.EMPTY_A, R.EMPTY_B)):
            assert p in pairs
        for flags in (0, EMPTY_NAN):
            want = sets.pairs(rows, cols, method=SORTED, flags=flags)
            got = check(sets, sets, *R.pairs_ref(*R.recipe_matrices(flags), rows, cols), rows, cols, flags)
            assert same_bytes(want, got)
    finally:
        sets.free()


# 4 ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["plain", "empty_nan"])
def test_equals_cross_matrix_and_concat_route(subj, qry, flags):
    rows, cols = P.lists()["mixed"]
    got = check(qry, subj, *P.pairs_ref(flags, rows, cols), rows, cols, flags)
    mI, mD = subj.cross_matrix(qry, flags=flags)
    assert same_bytes(got, (mI[rows, cols], mD[rows, cols]))
    both = subj.concat(qry)
    try:
        assert same_bytes(got, both.pairs(rows + NS, cols, method=SORTED, flags=flags))
    finally:
        both.free()


# 5 ---------------------------------------------------------------------------
def test_foreign_cut(ctx):
    """A query cut by splitters that were never its own: 20,000 codes in one
    subject segment (sub-runs of 4,096 staged keys), a query below every
    splitter with code 0, a query above every splitter with the all-ones code,
    the empty query."""
    import gdist
    S, Q = P.foreign_cut()
    subj = gdist.KmerSets.from_codes(S[0], S[1], 8, gdist.KmerType.PROT, ctx)
    qry = gdist.KmerSets.from_codes(Q[0], Q[1], 8, gdist.KmerType.PROT, ctx)
    try:
        rng = np.random.default_rng(12)
        r, c = np.divmod(np.arange(P.FC_NQ * P.FC_NS), P.FC_NS)
        rows = np.concatenate([r, rng.integers(0, P.FC_NQ, 8)])
        cols = np.concatenate([c, rng.integers(0, P.FC_NS, 8)])
        for flags in (0, EMPTY_NAN):
            eI, eD = P.foreign_cut_expected(flags)
            check(qry, subj, eI[rows, cols], eD[rows, cols], rows, cols, flags)
        p = rng.permutation(len(rows))
        check(qry, subj, eI[rows[p], cols[p]], eD[rows[p], cols[p]], rows[p], cols[p], EMPTY_NAN)
        # one pair at a time: a unit of one column splits the run over its waves
        for i, j in ((0, 1), (0, 4), (1, 0), (2, 0), (3, 0)):
            check(qry, subj, eI[[i], [j]], eD[[i], [j]], [i], [j], EMPTY_NAN)
        mI, mD = subj.cross_matrix(qry, flags=EMPTY_NAN)
        assert np.array_equal(mI, eI) and np.array_equal(mD.view(np.uint64), eD.view(np.uint64))
    finally:
        qry.free()
        subj.free()


# 6 ---------------------------------------------------------------------------
def test_large_sets_are_cut(ctx):
    import gdist
    from gdist import synth
    seqs = [bytes(r) for r in synth.genomes(4, 250_000, 0.02, 9)]
    off, codes = oracle.pack(seqs, 21, 0, 0)
    assert np.diff(off).min() > 400_000
    rows, cols = np.array([0, 0, 1, 1]), np.array([0, 1, 0, 1])
    eI, eD = pairs_ref.pairs_brute(off, codes, rows + 2, cols)
    assert eI.min() > 1000
    subj = gdist.KmerSets.from_sequences(seqs[:2], 21, gdist.KmerType.DNA, 0, ctx)
    qry = gdist.KmerSets.from_sequences(seqs[2:], 21, gdist.KmerType.DNA, 0, ctx)
    try:
        check(qry, subj, eI, eD, rows, cols)
        _, groups, units = qry.pairs_info()
        assert groups == 2 and units > groups, (groups, units)              # the cut path ran
    finally:
        qry.free()
        subj.free()


# 7 ---------------------------------------------------------------------------
def test_subjects_untouched(ctx, qry):
    import gdist
    res = gdist.KmerSets.from_sequences(X.sequences()[0], 21, gdist.KmerType.DNA, 0, ctx)
    try:
        res.build_bitsets()
        state = lambda: (res.bitset_info(), res.rare_info(), res.sparse_info(), res.build_timing(), len(res),
                         res.info())
        before = state()
        bI, bD = res.matrix((3, 40), (60, NS), method=gdist.METHOD_BITSET)
        rows, cols = P.lists()["mixed"]
        check(qry, res, *P.pairs_ref(0, rows, cols), rows, cols)
        assert state() == before
        aI, aD = res.matrix((3, 40), (60, NS), method=gdist.METHOD_BITSET)
        assert np.array_equal(aI, bI) and np.array_equal(aD.view(np.uint64), bD.view(np.uint64))
        assert state() == before
    finally:
        res.free()


# 8 ---------------------------------------------------------------------------
@pytest.mark.parametrize("flags", [0, SKETCH_JACCARD, EMPTY_NAN | SKETCH_JACCARD])
def test_sketches_take_the_sketch_pairs_route(subj, qry, flags):
    sks, skq = subj.sketches(64), qry.sketches(64)
    try:
        rows, cols = P.lists()["mixed"]
        want = skq.pairs(rows, cols, other=sks, flags=flags)
        info = skq.pairs_info()
        got = answer(skq, sks, rows, cols, flags)
        assert same_bytes(want, got)
        assert skq.pairs_info()[1:] == info[1:]
        assert int((got[0] > 0).sum()) > 0                   # some signatures share hashes
    finally:
        sks.free()
        skq.free()


# 9 ---------------------------------------------------------------------------
def test_einval_leaves_outputs_untouched(ctx, subj, qry):
    import gdist
    rows, cols = np.array([3, 4, 5], np.int64), np.array([9, 4, 0], np.int64)
    Null = types.SimpleNamespace(h=None, ctx=ctx)

    def refused(msg, q=qry, s=subj, r=rows, c=cols, **kw):
        rc, I, D = raw(q, s, r, c, **kw)
        assert rc == -1, (msg, rc)
        assert untouched(I, D), msg
        assert msg in last_error(), (msg, last_error())

    refused("null sets handle", q=Null)
    refused("null sets handle", s=Null)
    other = gdist.Context(0)
    foreign = gdist.KmerSets.from_sequences(X.sequences()[1][:6], 21, gdist.KmerType.DNA, 0, other)
    sk = subj.sketches(64)
    k15 = gdist.KmerSets.from_sequences(X.sequences()[1][:6], 15, gdist.KmerType.DNA, 0, ctx)
    prot = gdist.KmerSets.from_sequences([b"MKVLAAGIVGLLLAQ"] * 6, 8, gdist.KmerType.PROT, 0, ctx)
    bare = gdist.KmerSets.from_sequences(X.sequences()[0][:10], 21, gdist.KmerType.DNA, 0, ctx)
    bare.build_bitsets()
    bare.release_codes()
    try:
        refused("context", q=foreign)                        # different contexts
        refused("context", s=foreign)
        refused("context", ctx=other)                        # both of another context
        refused("kmer sets", q=sk)                           # one sketch collection, one of kmer sets
        refused("kmer sets", s=sk)
        for odd in (k15, prot):
            refused("different kmer specs", q=odd)
            refused("different kmer specs", s=odd)
        refused("no codes", q=bare)
        refused("no codes", s=bare)
        refused("GDIST_SKETCH_JACCARD", q=sk, s=sk, flags=UPPER_TRIANGLE)
    finally:
        for h in (foreign, sk, k15, prot, bare):
            h.free()
        other.close()
    refused("npairs outside", npairs=-1)
    refused("npairs outside", npairs=1 << 31)
    refused("null rows or cols", null=("rows",))
    refused("null rows or cols", null=("cols",))
    refused("both outputs null", null=("I", "D"))
    for flags in (UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF, SKETCH_JACCARD, EMPTY_NAN | UPPER_TRIANGLE):
        refused("GDIST_EMPTY_NAN", flags=flags)
    refused("row index outside the query collection", r=np.array([3, NQ, 5], np.int64))
    refused("row index outside the query collection", r=np.array([3, 4, -1], np.int64))
    refused("column index outside the subject collection", c=np.array([9, NS, 0], np.int64))
    refused("column index outside the subject collection", c=np.array([-1, 4, 0], np.int64))
    # rows are held to the queries' range, not the subjects': NQ <= NS - 1 < NS
    refused("row index outside the query collection", r=np.array([NS - 1, 4, 5], np.int64))
    # the empty list: nothing is read, nothing is touched
    from gdist import _lib as L
    assert L.lib.gdist_cross_pairs(ctx.h, qry.h, subj.h, 0, None, None, 0, None, None) == 0
    assert qry.pairs_info() == (-1.0, 0, 0)
    rc, I, D = raw(qry, subj, [], [], null=("rows", "cols"))
    assert rc == 0 and untouched(I, D)


# 10 --------------------------------------------------------------------------
def test_python_surface(ctx, subj, qry):
    import gdist
    rows, cols = P.lists()["unit_edges"]
    base = answer(qry, subj, rows, cols)
    assert same_bytes(base, qry.pairs(rows, cols, other=subj))
    assert same_bytes(base, qry.pairs(rows, cols, SORTED, 0, True, True, other=subj))
    I, D = qry.pairs(rows, cols, want_I=False, other=subj)
    assert I is None and same_bytes((base[1],), (D,))
    I, D = qry.pairs(rows, cols, want_D=False, other=subj)
    assert D is None and same_bytes((base[0],), (I,))
    I, D = qry.pairs([], [], other=subj)
    assert len(I) == len(D) == 0
    with pytest.raises(ValueError):
        qry.pairs(rows, cols, method=BITSET, other=subj)
    with pytest.raises(TypeError):
        qry.pairs(rows, cols, AUTO, 0, True, True, subj)        # `other` is keyword-only
    # one cell across two collections: the concat route's value, without the concat
    dq, ds = P.duplicate_pair()
    both = qry.concat(subj)
    try:
        for i, j in ((dq, ds), (7, 3), (P.EMPTY_Q, P.KMERLESS_S), (P.EMPTY_Q, 0)):
            want_d = float(both.row_query(i, [NQ + j])[0])
            wI, _ = both.matrix((i, i + 1), (NQ + j, NQ + j + 1), want_D=False)
            d = qry[i].distance(subj[j])
            assert np.float64(d).view(np.uint64) == np.float64(want_d).view(np.uint64), (i, j, d, want_d)
            assert qry[i].similarity(subj[j]) == int(wI[0, 0])
            assert subj[j].distance(qry[i]) == d and subj[j].similarity(qry[i]) == int(wI[0, 0])
        assert qry[dq].distance(subj[ds]) == 0.0
    finally:
        both.free()
