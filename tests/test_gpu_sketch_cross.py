"""Query sketches against a resident sketch collection on the device
(gdist_cross_* on two GDIST_SKETCH collections; csrc/sketch_cross.hip): the
reference's find / mash workload, one getClosest per incoming genome against a
MinHash database. The matrix is compared with the oracle's sketch_distance cell
by cell; the five calls with their one-collection twins on
gdist_sets_concat(subjects, queries); the LSH bucket query with the exact list.
Every comparison is bit for bit: integers with array_equal, distances through
their uint64 view. Outputs of refused calls are pre-filled with poison."""
import ctypes as C
import io

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

UPPER_TRIANGLE, OUT_DEVICE, EMPTY_NAN, SKETCH_JACCARD, KEEP_SELF = 0x100, 0x200, 0x400, 0x800, 0x1000
ALL_FLAGS = (0, SKETCH_JACCARD, EMPTY_NAN, SKETCH_JACCARD | EMPTY_NAN)
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
NSUBJ, NQRY = 70, 33   # 70 columns: more than a wave, more than a run of subjects, a ragged last run


def bits(a):
    return np.ascontiguousarray(a, dtype=np.float64).view(np.uint64)


def sig(values):
    return np.array(sorted(set(int(v) for v in values)), dtype=np.int32)


def random_sig(rng, n, lo, hi):
    """n distinct int32 of [lo, hi), ascending."""
    n = min(n, hi - lo)
    return sig(lo + rng.choice(hi - lo, size=n, replace=False)) if n else np.zeros(0, np.int32)


def edge_sigs(rng, width):
    """The signatures a segmented merge can get wrong, none longer than width:
    empty, the extreme hashes, lengths 1, 2, 5, width / 2 and width, all below /
    all above the random ones, interleaved, and a shared one (identical pair)."""
    w = width
    dense = lambda n: random_sig(rng, n, -2 * w, 2 * w + 8)
    out = [np.zeros(0, np.int32), sig([INT_MIN]), sig([INT_MAX]), sig([INT_MIN, INT_MAX][:w]),
           dense(1), dense(2), dense(5), dense(w // 2), dense(w),
           sig(range(-10 * w - 5, -9 * w - 5)),            # w hashes below every dense one
           sig(range(9 * w, 10 * w)),                      # and above
           sig(range(0, 2 * w, 2)), sig(range(1, 2 * w, 2)), sig(range(0, 3 * w, 3)),   # interleaved
           sig(list(dense(max(w - 2, 0))) + [INT_MIN, INT_MAX])[:w],
           sig(range(-w // 2, w - w // 2))]                # shared by both sides: an identical pair
    return [s[:w] for s in out]


def make_sides(width, seed):
    rng = np.random.default_rng(seed)
    subj = edge_sigs(rng, width)
    qry = edge_sigs(rng, width)
    while len(subj) < NSUBJ:
        n = int(rng.integers(0, width + 1))
        # every third one long against short ones: na < 64 < nb for the wide widths
        subj.append(random_sig(rng, width if len(subj) % 3 == 0 else n, -2 * width, 2 * width + 8))
    while len(qry) < NQRY:
        n = int(rng.integers(0, min(width, 40) + 1))
        qry.append(random_sig(rng, width if len(qry) % 4 == 0 else n, -2 * width, 2 * width + 8))
    order = rng.permutation(NSUBJ)       # the edges among the random ones
    subj = [subj[i] for i in order]
    qry = qry[:NQRY]
    qry[0], qry[8] = qry[8], qry[0]       # row 0 (the one-row call) is a full signature, not the empty one
    return subj, qry


def expected(subj, qry, width, flags):
    I = np.zeros((len(qry), len(subj)), np.int32)
    D = np.zeros((len(qry), len(subj)), np.float64)
    for a, q in enumerate(qry):
        for b, s in enumerate(subj):
            D[a, b], I[a, b] = oracle.sketch_distance(q, s, width, flags)
    return I, D


def check_matrix(S, Q, exp, flags, rows=None, cols=None, tag=None):
    r0, r1 = rows or (0, len(Q))
    c0, c1 = cols or (0, len(S))
    I, D = S.cross_matrix(Q, rows=rows, cols=cols, flags=flags)
    eI, eD = exp[0][r0:r1, c0:c1], exp[1][r0:r1, c0:c1]
    assert np.array_equal(I, eI), (tag, flags, np.argwhere(I != eI)[:5])
    assert np.array_equal(bits(D), bits(eD)), (tag, flags, np.argwhere(bits(D) != bits(eD))[:5])


# ---------------------------------------------------------------- a. the matrix against the oracle
@pytest.mark.parametrize("width", [1, 64, 65, 130, 1000])
def test_cross_matrix_vs_oracle(ctx, width):
    import gdist
    subj, qry = make_sides(width, 1000 + width)
    S = gdist.SketchSets.from_signatures(subj, width, ctx)
    Q = gdist.SketchSets.from_signatures(qry, width, ctx)
    try:
        for flags in ALL_FLAGS:
            exp = expected(subj, qry, width, flags)
            if flags & EMPTY_NAN:
                assert np.isnan(exp[1]).any()          # empty x empty is among the cells
            for nrows in (1, 3, 33):
                check_matrix(S, Q, exp, flags, rows=(0, nrows), tag=(width, nrows))
            # one output at a time
            I, _ = S.cross_matrix(Q, flags=flags, want_D=False)
            _, D = S.cross_matrix(Q, flags=flags, want_I=False)
            assert np.array_equal(I, exp[0]) and np.array_equal(bits(D), bits(exp[1]))
    finally:
        S.free()
        Q.free()


def test_cross_matrix_wide_signatures(ctx):
    """Width 20,000: two signatures are past any LDS budget, the kernel searches
    and merges in global memory."""
    import gdist
    width = 20000
    rng = np.random.default_rng(7)
    subj = [random_sig(rng, n, -40000, 40000) for n in (20000, 20000, 9000, 63, 0)]
    qry = [random_sig(rng, n, -40000, 40000) for n in (20000, 17, 12000, 20000)]
    qry[3] = subj[1].copy()
    S = gdist.SketchSets.from_signatures(subj, width, ctx)
    Q = gdist.SketchSets.from_signatures(qry, width, ctx)
    try:
        for flags in (0, SKETCH_JACCARD | EMPTY_NAN):
            check_matrix(S, Q, expected(subj, qry, width, flags), flags)
    finally:
        S.free()
        Q.free()


def test_cross_matrix_built_sketches(ctx):
    """Sketches the library made itself (KmerSets.sketches): the recorded kmer
    spec passes check_same_spec, and sequences with fewer kmers than the width
    give signatures shorter than it."""
    import gdist
    from gdist import synth
    width = 64
    seqs = [bytes(r) for r in synth.genomes(17, 400, 0.1, 5)]
    seqs[3], seqs[14] = seqs[3][:40], seqs[14][:30]      # dwarves: fewer than 64 kmers
    sk, qk = (gdist.KmerSets.from_sequences(s, 21, gdist.KmerType.DNA, 0, ctx) for s in (seqs[:12], seqs[12:]))
    S, Q = sk.sketches(width), qk.sketches(width)
    try:
        so, sv = S.download()
        qo, qv = Q.download()
        subj = [sv[so[i]:so[i + 1]] for i in range(12)]
        qry = [qv[qo[i]:qo[i + 1]] for i in range(5)]
        assert min(len(s) for s in subj + qry) < width
        for flags in (0, SKETCH_JACCARD):
            check_matrix(S, Q, expected(subj, qry, width, flags), flags)
    finally:
        for h in (S, Q, sk, qk):
            h.free()


# ---------------------------------------------------------------- b. the twins on concat(subjects, queries)
TW, TNS, TNQ = 130, 14, 12
TROWS, TCOLS = (2, 11), (3, 13)            # 9 x 10, q0 > 0, c0 > 0
EDGES = np.append(np.linspace(0.0, 0.98, 50), 1.0)
QLABELS = np.array([[0, 1, 2, 0, 1, -1, 2, 0, 1, 2, 0, 1], [3, 3, 3, 3, 4, 4, 4, 4, 5, 5, 5, 5]], np.int32)
SLABELS = np.array([[0, 1, 2, 0, 1, 2, 0, -3, 2, 0, 1, 2, 0, 1], [3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4, 5, 3, 4]], np.int32)


@pytest.fixture(scope="module")
def twin(ctx):
    """Ragged sides (lengths 0 .. width, shared hashes) and their concat."""
    import gdist
    rng = np.random.default_rng(99)
    lens_s = [130, 0, 64, 65, 1, 130, 17, 100, 128, 2, 90, 130, 33, 5]
    lens_q = [130, 12, 0, 64, 129, 3, 130, 70, 1, 101, 66, 40]
    subj = [random_sig(rng, n, 0, 260) for n in lens_s]
    qry = [random_sig(rng, n, 0, 260) for n in lens_q]
    qry[6] = subj[5].copy()                  # distance 0
    S = gdist.SketchSets.from_signatures(subj, TW, ctx)
    Q = gdist.SketchSets.from_signatures(qry, TW, ctx)
    Cc = S.concat(Q)
    yield S, Q, Cc
    for h in (S, Q, Cc):
        h.free()


@pytest.mark.parametrize("walk", ["default", "4x4"])
@pytest.mark.parametrize("flags", [0, SKETCH_JACCARD | EMPTY_NAN])
def test_twin_identity(twin, opts, walk, flags):
    S, Q, Cc = twin
    if walk == "4x4":
        opts(closest_rows=4, closest_cols=4)
    ns = len(S)
    (q0, q1), (c0, c1) = TROWS, TCOLS
    trows = (ns + q0, ns + q1)
    # matrix
    I, D = S.cross_matrix(Q, rows=TROWS, cols=TCOLS, flags=flags)
    tI, tD = Cc.matrix(rows=trows, cols=TCOLS, flags=flags)
    assert np.array_equal(I, tI) and np.array_equal(bits(D), bits(tD))
    # closest
    for n, md in ((3, 0.9), (10, 1.0), (1, 0.3)):
        idx, d, cnt = S.cross_closest(Q, n, md, rows=TROWS, cols=TCOLS, flags=flags)
        tidx, td, tcnt = Cc.closest(n, md, rows=trows, cols=TCOLS, flags=flags, keep_self=True)
        assert np.array_equal(idx, tidx) and np.array_equal(bits(d), bits(td)) and np.array_equal(cnt, tcnt), (n, md)
    # within: complete, a capacity that cuts a row, capacity 0
    rp, col, d = S.cross_within(Q, 0.95, rows=TROWS, cols=TCOLS, flags=flags)
    trp, tcol, td = Cc.within(0.95, rows=trows, cols=TCOLS, flags=flags, keep_self=True)
    assert np.array_equal(rp, trp) and np.array_equal(col, tcol) and np.array_equal(bits(d), bits(td))
    assert rp[-1] > 12 and (np.diff(rp) > 1).any()
    cut = int(rp[3]) + 1 if rp[4] - rp[3] > 1 else int(rp[-1]) - 1      # inside a row
    for cap in (cut, 0):
        rp2, col2, d2 = S.cross_within(Q, 0.95, rows=TROWS, cols=TCOLS, flags=flags, capacity=cap)
        trp2, tcol2, td2 = Cc.within(0.95, rows=trows, cols=TCOLS, flags=flags, keep_self=True, capacity=cap)
        assert np.array_equal(rp2, trp2) and np.array_equal(rp2, rp), cap
        assert len(col2) == cap and np.array_equal(col2, tcol2) and np.array_equal(bits(d2), bits(td2)), cap
        assert np.array_equal(col2, col[:cap]) and np.array_equal(bits(d2), bits(d[:cap])), cap
    # group stats: the labels are slabels[t] followed by qlabels[t]
    tlab = np.concatenate([SLABELS, QLABELS], axis=1)
    g = S.cross_group_stats(Q, QLABELS, SLABELS, rows=TROWS, cols=TCOLS, flags=flags)
    tg = Cc.group_stats(tlab, rows=trows, cols=TCOLS, upper=False, flags=flags)
    assert g.tobytes() == tg.tobytes()
    assert sum(int(b) for b in g.bad) > 0                 # the negative labels are in the rectangle
    # histogram: without and with labels
    for lab in (None, (QLABELS, SLABELS)):
        h = S.cross_histogram(Q, EDGES, *(lab or (None, None)), rows=TROWS, cols=TCOLS, flags=flags)
        th = Cc.histogram(EDGES, None if lab is None else tlab, rows=trows, cols=TCOLS, upper=False, flags=flags)
        assert h.tobytes() == th.tobytes()
        assert np.array_equal(h.counts, th.counts) and np.array_equal(h.nans, th.nans)
        assert np.array_equal(h.bad, th.bad)
    # empty ranges behave as the twins' do
    for rows, cols in (((4, 4), TCOLS), (TROWS, (6, 6))):
        tr = (ns + rows[0], ns + rows[1])
        assert S.cross_group_stats(Q, QLABELS, SLABELS, rows=rows, cols=cols, flags=flags).tobytes() == \
            Cc.group_stats(tlab, rows=tr, cols=cols, upper=False, flags=flags).tobytes()
        assert S.cross_histogram(Q, EDGES, rows=rows, cols=cols, flags=flags).tobytes() == \
            Cc.histogram(EDGES, rows=tr, cols=cols, upper=False, flags=flags).tobytes()
        rpe, cole, _ = S.cross_within(Q, 0.95, rows=rows, cols=cols, flags=flags)
        trpe, tcole, _ = Cc.within(0.95, rows=tr, cols=cols, flags=flags, keep_self=True)
        assert np.array_equal(rpe, trpe) and len(cole) == len(tcole) == 0
        ie, de, ce = S.cross_closest(Q, 3, 0.9, rows=rows, cols=cols, flags=flags)
        tie, tde, tce = Cc.closest(3, 0.9, rows=tr, cols=cols, flags=flags, keep_self=True)
        assert np.array_equal(ie, tie) and np.array_equal(bits(de), bits(tde)) and np.array_equal(ce, tce)


def test_same_handle_is_keep_self(twin):
    """One handle as both collections: every cell counts, the diagonal too."""
    S = twin[0]
    n = len(S)
    I, D = S.cross_matrix(S)
    tI, tD = S.matrix()
    assert np.array_equal(I, tI) and np.array_equal(bits(D), bits(tD))
    idx, d, cnt = S.cross_closest(S, 4, 0.9)
    tidx, td, tcnt = S.closest(4, 0.9, keep_self=True)
    assert np.array_equal(idx, tidx) and np.array_equal(bits(d), bits(td)) and np.array_equal(cnt, tcnt)
    # a non-empty signature is its own nearest neighbour at distance 0
    full = [i for i in range(n) if I[i, i] > 0]
    assert full and all(idx[i, 0] == i and d[i, 0] == 0.0 for i in full)


# ---------------------------------------------------------------- c. refusals
POISON_I, POISON_D, POISON_IDX, POISON_CNT, POISON_BYTE = -7, 7.5, 0x5A5A5A5A5A5A5A5A, -9, 0x5A


def every_call(ctx, q, s, rows, cols, flags, null=False):
    """Each of the five calls into poisoned outputs: [(name, rc, message, the
    outputs still poisoned)]."""
    from gdist import _lib as L
    r0, r1 = rows
    c0, c1 = cols
    nr, nc = max(r1 - r0, 1), max(c1 - c0, 1)
    res = []

    def done(name, rc, *arrays):
        msg = L.lib.gdist_last_error().decode() if rc else ""
        clean = all(bool((a == p).all()) for a, p in arrays)
        res.append((name, rc, msg, clean))

    I = np.full((nr, nc), POISON_I, np.int32)
    D = np.full((nr, nc), POISON_D, np.float64)
    rc = L.lib.gdist_cross_matrix(ctx.h, q.h, s.h, r0, r1, c0, c1, flags, None if null else L.ptr(I, C.c_int32),
                                  None if null else L.ptr(D, C.c_double), nc)
    done("matrix", rc, (I, POISON_I), (D, POISON_D))
    idx = np.full((nr, 3), POISON_IDX, np.int64)
    d = np.full((nr, 3), POISON_D, np.float64)
    cnt = np.full(nr, POISON_CNT, np.int32)
    rc = L.lib.gdist_cross_closest(ctx.h, q.h, s.h, r0, r1, c0, c1, flags, 3, 0.9, L.ptr(idx, C.c_int64),
                                   L.ptr(d, C.c_double), None if null else L.ptr(cnt, C.c_int32))
    done("closest", rc, (idx, POISON_IDX), (d, POISON_D), (cnt, POISON_CNT))
    rp = np.full(nr + 1, POISON_CNT, np.int64)
    col = np.full(nr * nc, POISON_IDX, np.int64)
    dw = np.full(nr * nc, POISON_D, np.float64)
    total = C.c_int64(POISON_CNT)
    rc = L.lib.gdist_cross_within(ctx.h, q.h, s.h, r0, r1, c0, c1, flags, 0.9, nr * nc,
                                  None if null else L.ptr(rp, C.c_int64), L.ptr(col, C.c_int64),
                                  L.ptr(dw, C.c_double), C.byref(total))
    done("within", rc, (rp, POISON_CNT), (col, POISON_IDX), (dw, POISON_D),
         (np.array([total.value]), POISON_CNT))
    ql = np.zeros((1, max(len(q), 1)), np.int32)
    sl = np.zeros((1, max(len(s), 1)), np.int32)
    sides = np.full(2 * C.sizeof(L.GroupSide), POISON_BYTE, np.uint8)
    bad = np.full(1, POISON_CNT, np.int64)
    rc = L.lib.gdist_cross_group_stats(ctx.h, q.h, s.h, r0, r1, c0, c1, flags, 1, L.ptr(ql, C.c_int32),
                                       L.ptr(sl, C.c_int32), None if null else sides.ctypes.data,
                                       L.ptr(bad, C.c_int64))
    done("group_stats", rc, (sides, POISON_BYTE), (bad, POISON_CNT))
    e = np.array([0.25, 0.5], np.float64)
    counts = np.full((1, 3), POISON_CNT, np.int64)
    nans = np.full(1, POISON_CNT, np.int64)
    rc = L.lib.gdist_cross_histogram(ctx.h, q.h, s.h, r0, r1, c0, c1, flags, 2, L.ptr(e, C.c_double), 0, None, None,
                                     None if null else L.ptr(counts, C.c_int64), L.ptr(nans, C.c_int64), None)
    done("histogram", rc, (counts, POISON_CNT), (nans, POISON_CNT))
    return res


def test_refusals(ctx, twin):
    import gdist
    from gdist import _lib as L
    S, Q, _ = twin
    ns, nq = len(S), len(Q)
    rng = np.random.default_rng(3)
    narrow = gdist.SketchSets.from_signatures([random_sig(rng, 64, 0, 260)], 64, ctx)
    kmers = gdist.KmerSets.from_sequences([b"ACGTACGTTGCATGCATTGACCAGT" * 3] * 2, 21, gdist.KmerType.DNA, 0, ctx)
    other = gdist.Context(0)
    foreign = gdist.SketchSets.from_signatures([random_sig(rng, 100, 0, 260)], TW, other)

    def refused(needle, q, s, rows, cols, flags=0, c=ctx, null=False):
        for name, rc, msg, clean in every_call(c, q, s, rows, cols, flags, null):
            assert rc == L.EINVAL and needle in msg and clean, (needle, name, rc, msg, clean)

    try:
        refused("kmer sets", kmers, S, (0, 2), (0, ns))            # mixed kinds, either way round
        refused("kmer sets", Q, kmers, (0, nq), (0, 2))
        refused("different kmer specs", narrow, S, (0, 1), (0, ns))  # another width
        refused("context", foreign, S, (0, 1), (0, ns))
        refused("context", Q, foreign, (0, nq), (0, 1))
        refused("context", Q, S, (0, nq), (0, ns), c=other)
        for rows in ((-1, 2), (3, 2), (0, nq + 1)):
            refused("query range", Q, S, rows, (0, ns))
        for cols in ((-1, 2), (3, 2), (0, ns + 1)):
            refused("column range", Q, S, (0, nq), cols)
        refused("GDIST_SKETCH_JACCARD", Q, S, (0, nq), (0, ns), flags=UPPER_TRIANGLE)
        refused("GDIST_SKETCH_JACCARD", Q, S, (0, nq), (0, ns), flags=OUT_DEVICE | SKETCH_JACCARD)
        refused("GDIST_SKETCH_JACCARD", Q, S, (0, nq), (0, ns), flags=KEEP_SELF)
        refused("null", Q, S, (0, nq), (0, ns), null=True)
        # the kmer-set pair keeps its own flag rule
        name, rc, msg, clean = every_call(ctx, kmers, kmers, (0, 2), (0, 2), SKETCH_JACCARD)[0]
        assert rc == L.EINVAL and "no flag but GDIST_EMPTY_NAN" in msg and "SKETCH" not in msg and clean
    finally:
        for h in (narrow, kmers, foreign):
            h.free()
        other.close()


def test_cross_info_units(ctx, twin, opts):
    """units = the (query, subject) pairs merged, whatever the walk; the times
    are -1 unless option time_kernels is set, and the matrix call has no
    consumer kernel."""
    S, Q, _ = twin
    S.cross_closest(Q, 3, 0.9, rows=TROWS, cols=TCOLS)
    assert ctx.cross_info() == (-1.0, -1.0, 9 * 10)
    opts(closest_rows=4, closest_cols=4, time_kernels=1)
    S.cross_within(Q, 0.9)
    join, select, units = ctx.cross_info()
    assert units == TNQ * TNS and join > 0 and select > 0
    S.cross_matrix(Q, rows=(1, 2))
    join, select, units = ctx.cross_info()
    assert units == TNS and join > 0 and select == 0.0
    S.cross_histogram(Q, EDGES, rows=(4, 4))
    assert ctx.cross_info()[2] == 0


# ---------------------------------------------------------------- d. the LSH query against the exact list
def test_lsh_lists_are_filtered_exact_lists(ctx):
    import gdist
    from gdist import synth
    width, stages, buckets, seed, md = 100, 6, 40, 77, 0.9
    seqs = [bytes(r) for r in synth.genomes(208, 3000, 0.08, 31)]
    sk, qk = (gdist.KmerSets.from_sequences(s, 21, gdist.KmerType.DNA, 0, ctx) for s in (seqs[:200], seqs[196:204]))
    S, Q = sk.sketches(width), qk.sketches(width)
    lsh = gdist.LSHIndex(S, stages, buckets, seed=seed)
    try:
        so, sv = S.download()
        qo, qv = Q.download()
        ssig = [sv[so[i]:so[i + 1]] for i in range(200)]
        qsig = [qv[qo[i]:qo[i + 1]] for i in range(8)]
        sb = [oracle.lsh_buckets(s, stages, buckets, seed) for s in ssig]
        got = lsh.getClosest(Q, 200, md)
        rp, col, d = S.cross_within(Q, md)
        assert sum(len(g) for g in got) > 8          # the query finds more than the four it shares with the subjects
        for a in range(8):
            exact = {int(c): float(x) for c, x in zip(col[rp[a]:rp[a + 1]], d[rp[a]:rp[a + 1]])}
            for c, x in got[a]:
                assert c in exact and bits([x])[0] == bits([exact[c]])[0], (a, c)
            qb = oracle.lsh_buckets(qsig[a], stages, buckets, seed)
            cand = {j for j in range(200) if any(x == y for x, y in zip(sb[j], qb))}
            # the exact list in (d, index) order, filtered to the bucket candidates
            want = sorted((x, c) for c, x in exact.items() if c in cand)
            assert [(c, x) for x, c in want] == got[a], a
    finally:
        lsh.free()
        for h in (S, Q, sk, qk):
            h.free()


# ---------------------------------------------------------------- e. find over a sketch database
def test_find_genomes_on_sketches(ctx):
    import gdist
    from gdist import synth
    from gdist.javafmt import java_format_f
    from gdist.processors import Genome, find_genomes
    width = 100
    seqs = [bytes(r) for r in synth.genomes(30, 2000, 0.08, 31)]
    mk = lambda pre, ss: [Genome(f"{pre}{i}.1", f"{pre} genome {i}", [s.decode()]) for i, s in enumerate(ss)]
    subjects, queries = mk("S", seqs[:24]), mk("Q", seqs[20:])
    sk = gdist.KmerSets.from_sequences([g.kmer_text() for g in subjects], 21, gdist.KmerType.DNA, 0, ctx)
    qk = gdist.KmerSets.from_sequences([g.kmer_text() for g in queries], 21, gdist.KmerType.DNA, 0, ctx)
    db, Q = sk.sketches(width), qk.sketches(width)
    Cc = db.concat(Q)
    try:
        for flags in (0, SKETCH_JACCARD):
            out = io.StringIO()
            found, fail = find_genomes(db, subjects, iter(queries), out, 5, 0.9, batch=4, kmer_size=21, flags=flags)
            idx, d, cnt = Cc.closest(5, 0.9, rows=(24, 34), cols=(0, 24), flags=flags, keep_self=True)
            lines = ["genome_id\tgenome_name\tneighbor_id\tneighbor_name\tdistance"]
            for a, q in enumerate(queries):
                for r in range(cnt[a]):
                    s = subjects[int(idx[a, r])]
                    lines.append(f"{q.id}\t{q.name}\t{s.id}\t{s.name}\t{java_format_f(float(d[a, r]), 8, 3)}")
            assert out.getvalue() == "\n".join(lines) + "\n"
            assert (found, fail) == (int(cnt.sum()), int((cnt == 0).sum()))
            assert found >= 4                           # the four shared genomes find themselves
        with pytest.raises(ValueError, match="kmer_size"):
            find_genomes(db, subjects, iter(queries), io.StringIO())
    finally:
        for h in (db, Q, Cc, sk, qk):
            h.free()
