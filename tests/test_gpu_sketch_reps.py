"""Greedy representatives of a sketch collection on the device
(gdist_sketch_greedy_reps; csrc/sketch_reps.hip over the column-list launch of
the ring kernel, csrc/sketch.hip). Every answer is compared with the
sequential loop over the oracle's distances (sketch_reps_ref): is_rep and
rep_of equal, rep_dist equal as uint64 views, and gdist_ctx_reps_info's cells
equal the count that says only representatives were merged. Outputs handed
over through ctypes are pre-filled with poison. One collection is uploaded a
width; the references are computed once."""
import ctypes as C
import io

import numpy as np
import pytest

import sketch_pairs_ref as P
import sketch_reps_ref as R
from sketch_reps_ref import ALL_FLAGS, BLOCK, EMPTY_NAN, SKETCH_JACCARD, UPPER_TRIANGLE, bits

pytestmark = pytest.mark.gpu

POISON_I, POISON_L, POISON_D = -7, -77, 7.5


@pytest.fixture(scope="module")
def handles(ctx):
    """width -> sketch_reps_ref.collection(width) on the device, uploaded on first use."""
    import gdist
    made = {}

    def get(width):
        if width not in made:
            made[width] = gdist.SketchSets.from_signatures(list(R.collection(width)[0]), width, ctx)
        return made[width]
    yield get
    for S in made.values():
        S.free()


def same(got, exp, tag):
    """(is_rep, rep_of, rep_d) equal the reference's, the distances bit for bit."""
    assert np.array_equal(got[0], exp[0]), (tag, np.flatnonzero(got[0] != exp[0])[:8])
    bad = np.flatnonzero(got[1] != exp[1])
    assert len(bad) == 0, (tag, bad[:8], got[1][bad[:8]], exp[1][bad[:8]])
    bad = np.flatnonzero(bits(got[2]) != bits(exp[2]))
    assert len(bad) == 0, (tag, bad[:8], got[2][bad[:8]], exp[2][bad[:8]])


def run(ctx, S, t, exp, block, flags=0, tie_rank=None, tag=None):
    """greedy_reps without and with assignment against exp, reps_info both times;
    block: the row block in force (reps_block, or N when unset)."""
    is_rep = S.greedy_reps(t, flags=flags)
    assert is_rep.dtype == np.int32 and np.array_equal(is_rep, exp[0]), (tag, np.flatnonzero(is_rep != exp[0])[:8])
    assert ctx.reps_info() == R.info(exp[0], block, False), tag
    got = S.greedy_reps(t, assign=True, tie_rank=tie_rank, flags=flags)
    same(got, exp, tag)
    assert ctx.reps_info() == R.info(exp[0], block, True), tag
    return got


# ---------------------------------------------------------------- 1. the main sweep
@pytest.mark.parametrize("width", R.WIDTHS)
def test_sweep_vs_oracle(ctx, handles, opts, width):
    S = handles(width)
    opts(reps_block=BLOCK)
    for flags in ALL_FLAGS:
        for t in R.thresholds(width, flags):
            run(ctx, S, t, R.case(width, flags, t), BLOCK, flags, tag=(width, flags, t))


# ---------------------------------------------------------------- 2. block sizes
@pytest.mark.parametrize("block", [None, 1, 32, 37, 70, 128])
def test_block_sizes(ctx, handles, opts, block):
    """Unset (one block), 1 (every decision through the column-list kernel), 32,
    37 (off the 32-wide tile), 70 and 128: one result."""
    width = 65
    S = handles(width)
    n = len(S)
    if block is not None:
        opts(reps_block=block)
    for flags in (0, SKETCH_JACCARD | EMPTY_NAN):
        for t in R.thresholds(width, flags)[1:3]:
            run(ctx, S, t, R.case(width, flags, t), min(block or n, n), flags, tag=(block, flags, t))


# ---------------------------------------------------------------- 3. tie rank
def test_tie_rank(ctx, handles, opts):
    flags, t, exp = R.tie_case(64)
    S = handles(64)
    for block in (BLOCK, None):
        opts(reps_block=block)
        for name, rank in R.tie_ranks(len(S)).items():
            run(ctx, S, t, exp[name], block or len(S), flags, tie_rank=rank, tag=(name, block))


# ---------------------------------------------------------------- 4. edge thresholds
@pytest.mark.parametrize("width", [1, 65])
def test_edge_thresholds(ctx, handles, opts, width):
    S = handles(width)
    n = len(S)
    opts(reps_block=BLOCK)
    for flags in ALL_FLAGS:
        D = R.expected(width, flags)
        # -1.0: every set is a representative
        exp = R.greedy(D, -1.0)
        assert exp[0].all()
        run(ctx, S, -1.0, exp, BLOCK, flags, tag=(width, flags, -1.0))
        # 0.0: identical signatures only; past width 1 those are the three copies
        exp = R.greedy(D, 0.0)
        if width > 1:
            assert list(np.flatnonzero(exp[0] == 0)) == [n - 3, n - 2, n - 1]
            assert list(exp[1][n - 3:]) == list(R.collection(width)[1])
        run(ctx, S, 0.0, exp, BLOCK, flags, tag=(width, flags, 0.0))
    # 1.0 and +inf: d == 1.0 covers, NaN never does (an empty signature first,
    # another one last: under GDIST_EMPTY_NAN the last is a representative too)
    import gdist
    N = gdist.SketchSets.from_signatures(list(R.nan_collection(width)), width, ctx)
    empties = sum(1 for s in R.nan_collection(width) if len(s) == 0)
    try:
        for flags in ALL_FLAGS:
            D = R.nan_expected(width, flags)
            for t in (1.0, float("inf")):
                exp = R.greedy(D, t)
                assert exp[0][0] == 1 and exp[0][-1] == (1 if flags & EMPTY_NAN else 0)
                assert exp[0].sum() == (empties if flags & EMPTY_NAN else 1)
                run(ctx, N, t, exp, BLOCK, flags, tag=(width, flags, t))
    finally:
        N.free()


# ---------------------------------------------------------------- 5. small sizes
@pytest.mark.parametrize("n", [1, 33])
def test_small(ctx, opts, n):
    import gdist
    width = 65
    sigs = list(R.collection(width)[0][:n])
    D = R.expected(width, 0)[:n, :n]
    S = gdist.SketchSets.from_signatures(sigs, width, ctx)
    try:
        for block in (None, BLOCK):
            opts(reps_block=block)
            for t in (-1.0, R.thresholds(width, 0)[2], 2.0):
                run(ctx, S, t, R.greedy(D, t), min(block or n, n), tag=(n, block, t))
    finally:
        S.free()


# ---------------------------------------------------------------- 6. wide signatures
def test_wide_signatures(ctx, opts):
    """The ring streams a signature: 20,000 hashes are no other path."""
    import gdist
    width = 20000
    sigs = P.wide_sides()[0]
    D = R.matrix_of(sigs, width, 0)
    t = float(np.sort(R.off_diagonal(D))[2])
    exp = R.greedy(D, t)
    assert 1 < exp[0].sum() < len(sigs)
    S = gdist.SketchSets.from_signatures(sigs, width, ctx)
    try:
        for block in (None, 2):
            opts(reps_block=block)
            run(ctx, S, t, exp, block or len(sigs), tag=("wide", block))
    finally:
        S.free()


# ---------------------------------------------------------------- 7. built sketches
def test_built_sketches(ctx, opts):
    """120 synthetic genomes sketched at width 200 on the device against the
    loop over the oracle's signatures; fasta_reps(sketch_width=200) prints that
    loop's lines."""
    import gdist
    from gdist import processors
    seqs, D = R.built()
    t = float(np.quantile(R.off_diagonal(D), 0.3, method="lower"))
    exp = R.checked(D, t, BLOCK)
    opts(reps_block=BLOCK)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sk = sets.sketches(200)
    try:
        run(ctx, sk, t, exp, BLOCK, tag="built")
    finally:
        sk.free()
        sets.free()
    recs = [gdist.Sequence("g%d" % i, "genome %d" % i, s.decode()) for i, s in enumerate(seqs)]
    out = io.StringIO()
    reps = processors.fasta_reps(recs, out, kmer_size=21, max_dist=t, ctx=ctx, sketch_width=200)
    want = [int(i) for i in np.flatnonzero(exp[0])]
    assert reps == want
    assert out.getvalue() == "seq\tname\n" + "".join("g%d\tgenome %d\n" % (i, i) for i in want)


def test_distance_reps_on_sketches(ctx, opts):
    """distance_reps(sketch_width=200): list.tbl equals the loop over the
    oracle's signatures, pass 2's ties by repMap's HashMap order; with a
    repeated id both passes go through row queries on the sketches."""
    import pyref
    from gdist import processors as procs
    seqs, D = R.built()
    n = len(seqs)
    t = float(np.quantile(R.off_diagonal(D), 0.3, method="lower"))
    assert 0.0 < t < 1.0
    opts(reps_block=BLOCK)
    ids = ["fig|%d.peg.%d" % (1000 + 37 * i, i) for i in range(n)]
    gens = [procs.Genome(ids[i], "n%d" % i, [s.decode()]) for i, s in enumerate(seqs)]
    reps = [int(i) for i in np.flatnonzero(R.checked(D, t, BLOCK)[0])]
    order = [reps[o] for o in procs.java_hashmap_order([ids[r] for r in reps], procs.DISTREPS_REPMAP_CAPACITY)]
    rank = np.full(n, n, np.int64)
    rank[order] = np.arange(len(order))
    _, rep_of, rep_d = R.greedy(D, t, rank)
    assert (rep_of >= 0).all()
    want = ["genome_id\tgenome_name\trep_id\trep_name\tdistance"] + [
        "%s\tn%d\t%s\tn%d\t%s" % (ids[i], i, ids[rep_of[i]], rep_of[i], pyref.java_double_str(float(rep_d[i])))
        for i in range(n)]
    prefix, lst, stats = procs.distance_reps(gens, kmer_size=21, max_dist=t, ctx=ctx, sketch_width=200)
    assert lst.splitlines() == want
    assert sum(int(l.split("\t")[2]) for l in stats.splitlines()[1:]) == n
    # a repeated id: the host loop with HashMap.put replacement, row queries on the sketches
    m = 12
    dup = [procs.Genome(ids[0] if i == 7 else ids[i], "n%d" % i, [seqs[i].decode()]) for i in range(m)]
    rep_of_key = {}
    for i, g in enumerate(dup):
        if not any(D[i, r] <= t for r in rep_of_key.values()):
            rep_of_key[g.id] = i
    dreps = list(rep_of_key.values())
    dorder = [dreps[o] for o in procs.java_hashmap_order([dup[r].id for r in dreps], procs.DISTREPS_REPMAP_CAPACITY)]
    want = []
    for i in range(m):
        if i in dreps:
            r, d = i, 0.0
        else:
            pos, d = P.argmin([D[i, c] for c in dorder])
            assert pos >= 0
            r = dorder[pos]
        want.append("%s\tn%d\t%s\tn%d\t%s" % (dup[i].id, i, dup[r].id, r, pyref.java_double_str(float(d))))
    _, lst, _ = procs.distance_reps(dup, kmer_size=21, max_dist=t, ctx=ctx, sketch_width=200)
    assert lst.splitlines()[1:] == want


# ---------------------------------------------------------------- 8. interleaving
def test_interleaved_with_matrix(ctx, handles, opts):
    width, flags = 1000, SKETCH_JACCARD
    S = handles(width)
    opts(reps_block=BLOCK)
    t = R.thresholds(width, flags)[1]
    exp = R.case(width, flags, t)
    first = run(ctx, S, t, exp, BLOCK, flags, tag="first")
    _, D = S.matrix(flags=flags)
    assert np.array_equal(bits(D), bits(R.expected(width, flags)))
    second = run(ctx, S, t, exp, BLOCK, flags, tag="second")
    for a, b in zip(first, second):
        assert np.array_equal(a.view(np.uint8), b.view(np.uint8))


# ---------------------------------------------------------------- 9. the ring's options
@pytest.mark.parametrize("ring", [dict(sketch_ring=16, sketch_cap=7), dict(sketch_ring=32, sketch_wait=1),
                                  dict(sketch_perm=0), dict(sketch_ring=512, sketch_cap=300)])
def test_ring_options(ctx, handles, opts, ring):
    """The column-list launch reads sketch_matrix's ring options: small rings
    (pairs that run ahead of a ring take the global-memory steps), waiting
    pairs, the plain slot addresses. One result."""
    width, flags = 1000, 0
    S = handles(width)
    opts(reps_block=BLOCK, **ring)
    t = R.thresholds(width, flags)[2]
    run(ctx, S, t, R.case(width, flags, t), BLOCK, flags, tag=ring)


# ---------------------------------------------------------------- 10. EINVAL
def test_einval_leaves_outputs(ctx, handles):
    import gdist
    from gdist import _lib as L
    S = handles(65)
    n = len(S)
    kset = gdist.KmerSets.from_sequences([b"ACGTACGTTTGACCAGTACGATCAGCATTTGACAGT" * 3] * 2, 21, gdist.KmerType.DNA, 0, ctx)

    def call(h, flags=0, null_is_rep=False):
        is_rep = np.full(n, POISON_I, np.int32)
        rep_of = np.full(n, POISON_L, np.int64)
        rep_d = np.full(n, POISON_D, np.float64)
        nreps = C.c_int64(POISON_L)
        rc = L.lib.gdist_sketch_greedy_reps(ctx.h, h, 0.5, flags, None, None if null_is_rep else L.ptr(is_rep, C.c_int32),
                                            L.ptr(rep_of, C.c_int64), L.ptr(rep_d, C.c_double), C.byref(nreps))
        clean = (is_rep == POISON_I).all() and (rep_of == POISON_L).all() and (rep_d == POISON_D).all() \
            and nreps.value == POISON_L
        return rc, bool(clean)

    try:
        before = ctx.reps_info()
        rc, clean = call(kset.h)
        assert rc == L.EINVAL and clean
        assert "gdist_greedy_reps" in L.lib.gdist_last_error().decode()
        assert call(S.h, flags=UPPER_TRIANGLE) == (L.EINVAL, True)
        assert call(S.h, null_is_rep=True) == (L.EINVAL, True)
        assert call(None) == (L.EINVAL, True)
        other = gdist.Context(0)                              # a handle of another context
        assert other.reps_info() == (0, 0, 0, 0)              # zeros before any call
        foreign = gdist.SketchSets.from_signatures(list(R.collection(65)[0]), 65, other)
        try:
            assert call(foreign.h) == (L.EINVAL, True)
            assert "another context" in L.lib.gdist_last_error().decode()
            foreign.greedy_reps(0.5)
            assert other.reps_info()[0] == 1 and ctx.reps_info() == before     # a context's own figures
        finally:
            foreign.free()
        assert ctx.reps_info() == before
        rc, clean = call(S.h)
        assert rc == 0 and not clean
        with pytest.raises(ValueError):
            S.greedy_reps(0.5, flags=UPPER_TRIANGLE)
    finally:
        kset.free()
