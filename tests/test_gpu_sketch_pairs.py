"""The sketch distances of a pair list in one device call (gdist_sketch_pairs;
csrc/sketch_pairs.hip): the methods table's (id1, id2) list, one genome against
a column list and the chosen pairs of the width comparison, on GDIST_SKETCH
collections. Every answer is compared bit for bit (array_equal on the common
counts, the fp64 bits of D) with the oracle's sketch_distance of the pair, with
the cell gdist_cross_matrix / gdist_sketch_matrix write, and with itself under a
permutation of the list. Outputs are 16 slots longer than the list and
pre-filled with poison: a slot the call leaves unwritten fails, a slot past the
list it touches fails too. The references are computed once (sketch_pairs_ref)."""
import ctypes as C
import io

import numpy as np
import pytest

import oracle
import sketch_pairs_ref as R
from sketch_pairs_ref import ALL_FLAGS, EMPTY_NAN, NQRY, NSUBJ, SKETCH_JACCARD, bits

pytestmark = pytest.mark.gpu

POISON_I, POISON_D, GUARD = -7, 7.5, 16


def last_error():
    from gdist import _lib as L
    return L.lib.gdist_last_error().decode()


def raw(ctx, a, b, rows, cols, flags=0, null=(), npairs=None):
    """gdist_sketch_pairs into poisoned outputs with GUARD slots past the list:
    (rc, common, D). `null`: the arguments handed over as NULL (of "a", "b",
    "rows", "cols", "common", "D")."""
    from gdist import _lib as L
    rows = np.ascontiguousarray(rows, np.int64)
    cols = np.ascontiguousarray(cols, np.int64)
    n = len(rows) if npairs is None else npairs
    common = np.full(len(rows) + GUARD, POISON_I, np.int32)
    D = np.full(len(rows) + GUARD, POISON_D, np.float64)
    rb = rows if len(rows) else np.zeros(1, np.int64)
    cb = cols if len(cols) else np.zeros(1, np.int64)
    rc = L.lib.gdist_sketch_pairs(ctx.h, None if "a" in null else a.h, None if "b" in null else b.h, n,
                                  None if "rows" in null else L.ptr(rb, C.c_int64),
                                  None if "cols" in null else L.ptr(cb, C.c_int64), flags,
                                  None if "common" in null else L.ptr(common, C.c_int32),
                                  None if "D" in null else L.ptr(D, C.c_double))
    return rc, common, D


def untouched(common, D):
    return bool(np.all(common == POISON_I) and np.all(D == POISON_D))


def check(ctx, a, b, exp, rows, cols, flags=0, null=(), tag=None):
    """The call equals the cells exp = (common, D)[rows, cols]; the slots past
    the list and a NULL output's array stay poison. Returns (common, D) cut to
    the list."""
    rc, common, D = raw(ctx, a, b, rows, cols, flags, null)
    assert rc == 0, (tag, last_error())
    n = len(rows)
    xI, xD = exp[0][rows, cols], exp[1][rows, cols]
    if "common" in null:
        assert np.all(common == POISON_I), tag
    else:
        bad = np.flatnonzero(common[:n] != xI)
        assert len(bad) == 0, (tag, flags, bad[:5], common[bad[:5]], xI[bad[:5]])
        assert np.all(common[n:] == POISON_I), tag
    if "D" in null:
        assert np.all(D == POISON_D), tag
    else:
        bad = np.flatnonzero(bits(D[:n]) != bits(xD))
        assert len(bad) == 0, (tag, flags, bad[:5], D[bad[:5]], xD[bad[:5]])
        assert np.all(D[n:] == POISON_D), tag
    return common[:n], D[:n]


@pytest.fixture(scope="module")
def handles(ctx):
    """width -> (S, Q): the subjects and queries of sketch_pairs_ref.sides on
    the device, uploaded on first use."""
    import gdist
    made = {}

    def get(width):
        if width not in made:
            subj, qry = R.sides(width)
            made[width] = (gdist.SketchSets.from_signatures(subj, width, ctx),
                           gdist.SketchSets.from_signatures(qry, width, ctx))
        return made[width]
    yield get
    for S, Q in made.values():
        S.free()
        Q.free()


# ---------------------------------------------------------------- 1. against the oracle
@pytest.mark.parametrize("width", R.WIDTHS)
def test_lists_vs_oracle(ctx, handles, width):
    S, Q = handles(width)
    for flags in ALL_FLAGS:
        exp = R.expected(width, flags)
        for name, (rows, cols) in R.lists().items():
            check(ctx, Q, S, exp, rows, cols, flags, tag=(width, name))
        rows, cols = R.lists()["rectangle"]
        if flags & EMPTY_NAN:
            assert np.isnan(exp[1][rows, cols]).any()      # empty x empty is in the list
        # one output at a time
        check(ctx, Q, S, exp, rows, cols, flags, null=("D",), tag=(width, "common only"))
        check(ctx, Q, S, exp, rows, cols, flags, null=("common",), tag=(width, "D only"))
    # through the class
    exp = R.expected(width, SKETCH_JACCARD)
    rows, cols = R.lists()["row_200"]
    common, D = Q.pairs(rows, cols, other=S, flags=SKETCH_JACCARD)
    assert np.array_equal(common, exp[0][rows, cols]) and np.array_equal(bits(D), bits(exp[1][rows, cols]))
    common, D = Q.pairs(rows, cols, other=S, flags=SKETCH_JACCARD, want_common=False)
    assert common is None and np.array_equal(bits(D), bits(exp[1][rows, cols]))
    common, D = Q.pairs(rows, cols, other=S, flags=SKETCH_JACCARD, want_D=False)
    assert D is None and np.array_equal(common, exp[0][rows, cols])


# ---------------------------------------------------------------- 2. the twins
@pytest.mark.parametrize("width", [65, 1000])
def test_twins(ctx, handles, width):
    S, Q = handles(width)
    subj, _ = R.sides(width)
    for flags in (0, SKETCH_JACCARD | EMPTY_NAN):
        # two collections: gdist_cross_matrix's cells
        tw = S.cross_matrix(Q, flags=flags)
        for name in ("rectangle", "row_65", "singles"):
            check(ctx, Q, S, tw, *R.lists()[name], flags, tag=(width, name))
        # one handle: gdist_sketch_matrix's cells, (i, j) next to (j, i), i == j
        # for a full and for an empty signature
        full = next(i for i, s in enumerate(subj) if len(s) == width)
        empty = next(i for i, s in enumerate(subj) if len(s) == 0)
        m = S.matrix(flags=flags)
        rng = np.random.default_rng(5)
        i, j = rng.integers(0, NSUBJ, 150), rng.integers(0, NSUBJ, 150)
        rows = np.concatenate([i, j, [full, empty, full, empty]])
        cols = np.concatenate([j, i, [full, empty, empty, full]])
        common, D = check(ctx, S, S, m, rows, cols, flags, tag=(width, "one handle"))
        assert np.array_equal(common[:150], common[150:300]) and np.array_equal(bits(D[:150]), bits(D[150:300]))
        assert common[300] == width and D[300] == 0.0
        assert common[301] == 0 and (np.isnan(D[301]) if flags & EMPTY_NAN else D[301] == 1.0)
        got = S.pairs(rows, cols, flags=flags)
        assert np.array_equal(got[0], common) and np.array_equal(bits(got[1]), bits(D))


# ---------------------------------------------------------------- 3. order independence and bounds
def test_order_independence(ctx, handles):
    width = 130
    S, Q = handles(width)
    exp = R.expected(width, EMPTY_NAN)
    rows, cols = R.runs_and_singles()
    base = check(ctx, Q, S, exp, rows, cols, EMPTY_NAN)
    again = check(ctx, Q, S, exp, rows, cols, EMPTY_NAN)                   # two runs
    assert np.array_equal(base[0], again[0]) and np.array_equal(bits(base[1]), bits(again[1]))
    p = np.random.default_rng(11).permutation(len(rows))
    got = check(ctx, Q, S, exp, rows[p], cols[p], EMPTY_NAN)
    assert np.array_equal(got[0], base[0][p]) and np.array_equal(bits(got[1]), bits(base[1][p]))
    # a pair's slot does not depend on the rest of the list
    sub = check(ctx, Q, S, exp, rows[:100], cols[:100], EMPTY_NAN)
    assert np.array_equal(sub[0], base[0][:100]) and np.array_equal(bits(sub[1]), bits(base[1][:100]))


# ---------------------------------------------------------------- 4. the global variant
def test_wide_signatures(ctx):
    """Width 20,000: (1 + 16) signatures are past the LDS budget, the kernel
    searches and merges in global memory."""
    import gdist
    width = 20000
    subj, qry = R.wide_sides()
    S = gdist.SketchSets.from_signatures(subj, width, ctx)
    Q = gdist.SketchSets.from_signatures(qry, width, ctx)
    rows, cols = (x.reshape(-1).astype(np.int64) for x in np.divmod(np.arange(20).reshape(4, 5), 5))
    try:
        for flags in (0, SKETCH_JACCARD | EMPTY_NAN):
            check(ctx, Q, S, R.rectangle(qry, subj, width, flags), rows, cols, flags, tag="wide")
    finally:
        S.free()
        Q.free()


@pytest.mark.parametrize("width", [1203, 1204])
def test_lds_boundary(ctx, width):
    """The widest signatures the LDS variant takes (one row beside the 16
    slices) and the first width of the global variant."""
    import gdist
    rng = np.random.default_rng(width)
    sigs = [R.random_sig(rng, n, -3000, 3000) for n in [width, width, 0, 1, 63, 64, 65, 600] + [width] * 4]
    sigs[9] = sigs[1].copy()
    S = gdist.SketchSets.from_signatures(sigs, width, ctx)
    rows, cols = (x.astype(np.int64) for x in np.divmod(rng.permutation(144), 12))
    try:
        for flags in (0, SKETCH_JACCARD | EMPTY_NAN):
            check(ctx, S, S, R.rectangle(sigs, sigs, width, flags), rows, cols, flags, tag=width)
    finally:
        S.free()


@pytest.mark.parametrize("width", [65, 1100])
def test_many_units(ctx, width):
    """Lists of thousands of units: a workgroup then holds several consecutive
    units a step (at most 4; 2 at width 1,100, where only two row signatures fit
    beside the slices) and deals their pairs to its waves as one run. The step
    size follows the list's units over the grid (two workgroups a CU), so the
    three lists are sized for 2, 3 and 4 units a step on 256 CUs; the unit
    counts asserted below are what puts them there."""
    import gdist
    n = 9000
    rng = np.random.default_rng(77 + width)
    vals = np.cumsum(rng.integers(1, 4, size=(n, 65), dtype=np.int32), axis=1, dtype=np.int32)
    lens = rng.integers(0, 66, n)
    sigs = [vals[i, :lens[i]] for i in range(n)]
    S = gdist.SketchSets.from_signatures(sigs, width, ctx)
    rows, cols = rng.integers(0, n, 40000), rng.integers(0, n, 40000)
    try:
        for npairs, lo, hi in ((6000, 4096, 6144), (11000, 6144, 8192), (40000, 8192, 1 << 30)):
            r, c = rows[:npairs], cols[:npairs]
            want = [oracle.sketch_distance(sigs[i], sigs[j], width, EMPTY_NAN) for i, j in zip(r, c)]
            rc, common, D = raw(ctx, S, S, r, c, EMPTY_NAN)
            assert rc == 0, last_error()
            assert np.array_equal(common[:npairs], [w[1] for w in want]), npairs
            assert np.array_equal(bits(D[:npairs]), bits([w[0] for w in want])), npairs
            assert np.all(common[npairs:] == POISON_I) and np.all(D[npairs:] == POISON_D)
            _, groups, units = S.pairs_info()
            assert groups == len(np.unique(r)) and units == R.unit_count(r) and lo <= units < hi, (npairs, units)
    finally:
        S.free()


# ---------------------------------------------------------------- 5. built sketches
def test_built_sketches(ctx):
    """Sketches the library made itself (KmerSets.sketches), two of them of
    dwarves (fewer kmers than the width), a list across two collections."""
    import gdist
    from gdist import synth
    width = 64
    seqs = [bytes(r) for r in synth.genomes(17, 400, 0.1, 5)]
    seqs[3], seqs[14] = seqs[3][:40], seqs[14][:30]
    sk, qk = (gdist.KmerSets.from_sequences(s, 21, gdist.KmerType.DNA, 0, ctx) for s in (seqs[:12], seqs[12:]))
    S, Q = sk.sketches(width), qk.sketches(width)
    try:
        so, sv = S.download()
        qo, qv = Q.download()
        subj = [sv[so[i]:so[i + 1]] for i in range(12)]
        qry = [qv[qo[i]:qo[i + 1]] for i in range(5)]
        assert len(subj[3]) < width and len(qry[2]) < width
        rng = np.random.default_rng(1)
        rows = np.concatenate([rng.integers(0, 5, 40), [2, 2, 0]]).astype(np.int64)
        cols = np.concatenate([rng.integers(0, 12, 40), [3, 11, 3]]).astype(np.int64)
        for flags in (0, SKETCH_JACCARD):
            check(ctx, Q, S, R.rectangle(qry, subj, width, flags), rows, cols, flags, tag="built")
    finally:
        for h in (S, Q, sk, qk):
            h.free()


# ---------------------------------------------------------------- 6. refusals
def test_refusals(ctx, handles):
    import gdist
    S, Q = handles(130)                           # 70 subjects, 33 queries
    rng = np.random.default_rng(3)
    narrow = gdist.SketchSets.from_signatures([R.random_sig(rng, 64, 0, 260)] * 3, 64, ctx)
    kmers = gdist.KmerSets.from_sequences([b"ACGTACGTTGCATGCATTGACCAGT" * 3] * 3, 21, gdist.KmerType.DNA, 0, ctx)
    other = gdist.Context(0)
    foreign = gdist.SketchSets.from_signatures([R.random_sig(rng, 100, 0, 260)] * 3, 130, other)
    rows, cols = np.array([0, 1, 2], np.int64), np.array([2, 1, 0], np.int64)

    def refused(needle, a=Q, b=S, r=rows, c=cols, cx=ctx, **kw):
        rc, common, D = raw(cx, a, b, r, c, **kw)
        assert rc == -1, (needle, rc)
        assert untouched(common, D), needle
        assert needle in last_error(), (needle, last_error())

    try:
        refused("null sets handle", null=("a",))
        refused("null sets handle", null=("b",))
        refused("another context", a=foreign)
        refused("another context", b=foreign)
        refused("another context", cx=other)
        refused("GDIST_SKETCH collections", a=kmers)
        refused("GDIST_SKETCH collections", b=kmers)
        refused("GDIST_SKETCH collections", a=kmers, b=kmers)
        refused("different kmer specs", a=narrow)
        refused("different kmer specs", b=narrow)
        refused("npairs outside", npairs=-1)
        refused("npairs outside", npairs=1 << 31)
        refused("null rows or cols", null=("rows",))
        refused("null rows or cols", null=("cols",))
        refused("both outputs null", null=("common", "D"))
        for flags in (R.UPPER_TRIANGLE, R.OUT_DEVICE | SKETCH_JACCARD, R.KEEP_SELF):
            refused("no flag but GDIST_EMPTY_NAN and GDIST_SKETCH_JACCARD", flags=flags)
        # each list against its own collection: NSUBJ - 1 indexes S, not Q
        refused("row index outside", r=np.array([0, NSUBJ - 1, 2], np.int64))
        refused("row index outside", r=np.array([0, 1, -1], np.int64))
        refused("row index outside", r=np.array([NQRY, 1, 2], np.int64))
        refused("column index outside", c=np.array([2, 1, NSUBJ], np.int64))
        refused("column index outside", c=np.array([-1, 1, 0], np.int64))
        refused("column index outside", a=S, b=Q, c=np.array([2, NSUBJ - 1, 0], np.int64))   # the mirror case
        refused("column index outside", a=S, b=Q, r=np.array([NSUBJ - 1, 1, 2], np.int64),
                c=np.array([2, NQRY, 0], np.int64))
        # the same indices are fine where they belong
        exp = R.expected(130, 0)
        check(ctx, Q, S, exp, np.array([NQRY - 1], np.int64), np.array([NSUBJ - 1], np.int64))
        check(ctx, S, Q, (exp[0].T, exp[1].T), np.array([NSUBJ - 1], np.int64), np.array([NQRY - 1], np.int64))
        # the empty list: OK, nothing touched, null lists allowed
        from gdist import _lib as L
        assert L.lib.gdist_sketch_pairs(ctx.h, Q.h, S.h, 0, None, None, 0, None, None) == 0
        rc, common, D = raw(ctx, Q, S, [], [])
        assert rc == 0 and untouched(common, D)
        rc, common, D = raw(ctx, Q, S, rows, cols, null=("rows", "cols"), npairs=0)
        assert rc == 0 and untouched(common, D)
        assert Q.pairs_info() == (-1.0, 0, 0)
        common, D = Q.pairs([], [], other=S)
        assert len(common) == len(D) == 0
    finally:
        for h in (narrow, kmers, foreign):
            h.free()
        other.close()


# ---------------------------------------------------------------- 7. info
def test_pairs_info(ctx, handles, opts):
    import gdist
    width = 130
    S, Q = handles(width)
    exp = R.expected(width, 0)
    rows, cols = R.runs_and_singles()
    runs = np.unique(rows, return_counts=True)[1]
    assert sorted(runs.tolist())[-4:] == [64, 65, 66, 201] and len(runs) == NQRY
    check(ctx, Q, S, exp, rows, cols)
    ms, groups, units = Q.pairs_info()
    assert ms == -1.0 and groups == NQRY
    assert units == R.unit_count(rows) == (NQRY - 4) + 1 + 2 + 2 + 4
    for name, (r, c) in R.lists().items():
        check(ctx, Q, S, exp, r, c)
        assert Q.pairs_info()[1:] == (len(np.unique(r)), R.unit_count(r)), name
    opts(time_kernels=1)
    check(ctx, Q, S, exp, rows, cols)
    ms, groups, units = Q.pairs_info()
    assert ms >= 0.0 and (groups, units) == (NQRY, R.unit_count(rows))
    opts(time_kernels=0)
    # a following gdist_pairs call on kmer sets reports its own numbers again
    kmers = gdist.KmerSets.from_sequences([b"ACGTACGTTGCATGCATTGACCAGT" * 3, b"TTGACCAGTACGTTGCATGCACGTA" * 3], 21,
                                          gdist.KmerType.DNA, 0, ctx)
    try:
        kmers.pairs([0, 0, 1], [1, 0, 1], method=gdist.METHOD_SORTED)
        assert kmers.pairs_info() == (-1.0, 2, 2)          # two rows, a unit each
    finally:
        kmers.free()


# ---------------------------------------------------------------- 8. row_query
def test_row_query(ctx, handles):
    import gdist
    width = 130
    S, Q = handles(width)
    subj, qry = R.sides(width)
    exp = R.expected(width, 0)
    # ALL equals the pair list, against a second collection
    cols = [5, 69, 0, 33, 5]
    d = Q.row_query(0, cols, gdist.QUERY_ALL, other=S)
    assert np.array_equal(bits(d), bits(exp[1][0, cols]))
    assert np.array_equal(bits(d), bits(Q.pairs([0] * 5, cols, other=S)[1]))
    close = False
    for q in range(NQRY):
        ds = exp[1][q]
        assert Q.row_query(q, range(NSUBJ), gdist.QUERY_ARGMIN, other=S) == R.argmin(ds), q
        for t in (0.0, 0.5, 0.97, 1.0):
            assert Q.row_query(q, range(NSUBJ), gdist.QUERY_ANY_LE, t, other=S) == R.any_le(ds, t), (q, t)
        close = close or R.argmin(ds)[0] >= 0
    assert close
    # a tie: the identical pair listed twice, the lowest position wins
    qi = next(i for i, s in enumerate(qry) if any(np.array_equal(s, x) for x in subj) and len(s) > 1)
    si = next(j for j, x in enumerate(subj) if np.array_equal(qry[qi], x))
    far = next(j for j in range(NSUBJ) if exp[1][qi, j] == 1.0)
    assert Q.row_query(qi, [far, si, far, si], gdist.QUERY_ARGMIN, other=S) == (1, 0.0)
    # a row where every distance is 1.0
    ones = [j for j in range(NSUBJ) if exp[1][qi, j] == 1.0]
    assert len(ones) > 1
    assert Q.row_query(qi, ones, gdist.QUERY_ARGMIN, other=S) == (-1, 1.0)
    assert Q.row_query(qi, ones, gdist.QUERY_ANY_LE, 0.99, other=S) is False
    assert Q.row_query(qi, ones, gdist.QUERY_ANY_LE, 1.0, other=S) is True
    # one collection
    e1 = S.matrix()[1]
    assert np.array_equal(bits(S.row_query(si, range(NSUBJ))), bits(e1[si]))
    assert S.row_query(si, range(NSUBJ), gdist.QUERY_ARGMIN) == R.argmin(e1[si])
    assert len(S.row_query(si, [])) == 0 and S.row_query(si, [], gdist.QUERY_ARGMIN) == (-1, 1.0)


# ---------------------------------------------------------------- 9. the methods mirror
def _genomes(n=12):
    from gdist import synth
    from gdist.processors import Genome
    dna = synth.genomes(n, 3000, 0.04, 17)
    return {f"{7000 + i}.{i + 1}": Genome(f"{7000 + i}.{i + 1}", f"Synthetic genome {i}", [bytes(dna[i]).decode()])
            for i in range(n)}


def test_minhash_method(ctx):
    from gdist import methods as M
    from gdist.javafmt import java_double
    genomes = _genomes()
    ids = list(genomes)
    rng = np.random.default_rng(9)
    pairs = [(ids[a], ids[b]) for a, b in zip(rng.integers(0, 12, 40), rng.integers(0, 12, 40))]
    pairs += [(ids[0], ids[j]) for j in range(1, 12)] + [pairs[0]]
    k, w = 15, 200
    off, codes = oracle.pack([genomes[i].kmer_text() for i in ids], k, 0, 0)
    ref = {i: oracle.sketch(codes[off[n]:off[n + 1]], k, 0, w) for n, i in enumerate(ids)}
    want = [oracle.sketch_distance(ref[a], ref[b], w, 0)[0] for a, b in pairs]
    assert 0 < sum(d < 1.0 for d in want) and len(set(want)) > 10
    m = M.DistanceMethod.create("minhash", ctx)
    m.parseParmString(f"K={k},W={w}")
    got = m.pair_distances([(genomes[a], genomes[b]) for a, b in pairs])
    assert np.array_equal(bits(got), bits(want))
    # one device pair-list call for the whole list
    firsts = [a for a, _ in pairs]
    assert m.pair_calls == 1
    assert m.last_info[1:] == (len(set(firsts)), R.unit_count([ids.index(a) for a in firsts]))
    # one first genome against its group
    meas = m.getMeasurer(genomes[ids[0]])
    group = [genomes[i] for i in ids[1:]]
    d = m.getDistances(meas, group)
    assert np.array_equal(bits(d), bits([oracle.sketch_distance(ref[ids[0]], ref[i], w, 0)[0] for i in ids[1:]]))
    assert m.pair_calls == 2 and m.last_info[1:] == (1, 1)
    m.prefetch(meas, group)
    assert m.pair_calls == 3 and m.getDistance(meas, group[4]) == d[4] and m.pair_calls == 3

    # the methods table: the exact kmer column and the sketch column
    def methods():
        return M.read_method_file(io.StringIO(f"type\tparms\nkmer\tK={k}\nminhash\tK={k},W={w}\n"), ctx)

    exact = methods()[0].pair_distances([(genomes[a], genomes[b]) for a, b in pairs])
    for whole in (True, False):
        ms = methods()
        out = io.StringIO()
        counts = M.method_table(pairs, ms, genomes, out, threads=4, whole_list=whole)
        lines = out.getvalue().splitlines()
        assert lines[0].split("\t")[5:] == [f"KMER_K{k}", f"MINHASH_K{k}_W{w}"]
        assert counts["pairs"] == len(pairs) == len(lines) - 1
        by_pair = {tuple(l.split("\t")[i] for i in (0, 2)): l.split("\t")[5:] for l in lines[1:]}
        for (a, b), e, s in zip(pairs, exact, want):
            assert by_pair[(a, b)] == [java_double(e), java_double(s)], (a, b)
        if whole:
            assert counts["device_calls"] == 2 and ms[1].pair_calls == 1
        else:
            assert ms[1].pair_calls == len(set(firsts))       # one call a first genome
