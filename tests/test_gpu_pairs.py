"""The distances of a pair list in one device call (gdist_pairs;
MethodTableProcessor.java:258-276). Every answer is compared with `==` (I, and
the fp64 bits of D) against the cells of the oracle's matrices (pairs_ref),
whatever the method, the order of the list and the tiers of the bitsets. The
outputs are pre-filled with garbage plus 3 guard slots past the list, so a slot
the call leaves unwritten fails and a guard slot it touches fails too. Each
property of a fixture a test relies on is asserted on the oracle's side first
(the lists' shapes: test_pairs_host.py)."""
import ctypes as C
import io
import itertools

import numpy as np
import pytest

import closest_ref as CR
import oracle
import pairs_ref as R
import refcache

pytestmark = pytest.mark.gpu

N = R.N
EMPTY_NAN, UPPER_TRIANGLE, OUT_DEVICE = 0x400, 0x100, 0x200
SORTED, BITSET, AUTO = 1, 2, 0
GARBAGE_I, GARBAGE_D = 0x5A5A5A5A, 7.5
METHODS = pytest.mark.parametrize("method", [SORTED, BITSET, AUTO], ids=["sorted", "bitset", "auto"])


def raw_pairs(sets, rows, cols, method=AUTO, flags=0, null=(), npairs=None):
    """gdist_pairs into garbage-filled outputs with 3 guard slots: (rc, I, D).
    `null`: the arguments handed over as NULL (of "rows", "cols", "I", "D")."""
    from gdist import _lib as L
    rows = np.ascontiguousarray(rows, np.int64)
    cols = np.ascontiguousarray(cols, np.int64)
    n = len(rows) if npairs is None else npairs
    I = np.full(len(rows) + 3, GARBAGE_I, dtype=np.int32)
    D = np.full(len(rows) + 3, GARBAGE_D, dtype=np.float64)
    rb = rows if len(rows) else np.zeros(1, np.int64)
    cb = cols if len(cols) else np.zeros(1, np.int64)
    rc = L.lib.gdist_pairs(sets.ctx.h, sets.h, n,
                           None if "rows" in null else L.ptr(rb, C.c_int64),
                           None if "cols" in null else L.ptr(cb, C.c_int64), method, flags,
                           None if "I" in null else L.ptr(I, C.c_int32),
                           None if "D" in null else L.ptr(D, C.c_double))
    return rc, I, D


def untouched(I, D):
    return bool(np.all(I == GARBAGE_I) and np.all(D == GARBAGE_D))


def check(sets, eI, eD, rows, cols, method=AUTO, flags=0, null=()):
    """The call equals pairs_ref on the oracle's whole matrices (eI, eD);
    returns (I, D) cut to the list."""
    rc, I, D = raw_pairs(sets, rows, cols, method, flags, null)
    assert rc == 0, last_error()
    n = len(rows)
    xI, xD = R.pairs_ref(eI, eD, rows, cols)
    if "I" in null:
        assert np.all(I == GARBAGE_I)
    else:
        bad = np.flatnonzero(I[:n] != xI)
        assert len(bad) == 0, (bad[:5], I[bad[:5]], xI[bad[:5]])
        assert np.all(I[n:] == GARBAGE_I)
    if "D" in null:
        assert np.all(D == GARBAGE_D)
    else:
        assert np.array_equal(D[:n].view(np.uint64), xD.view(np.uint64))
        assert np.all(D[n:] == GARBAGE_D)
    return I[:n], D[:n]


def last_error():
    from gdist import _lib as L
    return L.lib.gdist_last_error().decode()


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


@METHODS
@pytest.mark.parametrize("name", ["singletons", "long_group", "unit_edges", "mixed"])
def test_lists(kset, method, name):
    """The four list shapes; pairs_info's groups are the list's distinct rows,
    its units at least one per 64 pairs of a row (sorted), or one per pair (bitset)."""
    eI, eD = R.recipe_matrices()
    rows, cols = R.recipe_lists()[name]
    check(kset, eI, eD, rows, cols, method)
    ms, groups, units = kset.pairs_info()
    counts = np.unique(rows, return_counts=True)[1]
    assert groups == len(counts)
    assert ms == -1.0
    chunks = int(((counts + 63) // 64).sum())
    if method == SORTED:
        assert units >= chunks
    elif method == BITSET:
        assert units == len(rows)


@METHODS
def test_flags_and_self_pairs(kset, method):
    _, off, _, _ = CR.recipe()
    assert np.diff(off)[[R.EMPTY_A, R.EMPTY_B]].tolist() == [0, 0] and off[R.NONEMPTY + 1] > off[R.NONEMPTY]
    rows = np.array([R.EMPTY_A, R.EMPTY_A, R.EMPTY_B, R.NONEMPTY, R.NONEMPTY, R.EMPTY_B], np.int64)
    cols = np.array([R.EMPTY_A, R.EMPTY_B, R.EMPTY_A, R.NONEMPTY, R.EMPTY_A, 12], np.int64)
    I, D = check(kset, *R.recipe_matrices(EMPTY_NAN), rows, cols, method, EMPTY_NAN)
    assert np.isnan(D[:3]).all() and I[:3].tolist() == [0, 0, 0]
    assert I[3] == off[R.NONEMPTY + 1] - off[R.NONEMPTY] and D[3] == 0.0
    assert D[4:].tolist() == [1.0, 1.0]
    I, D = check(kset, *R.recipe_matrices(), rows, cols, method, 0)
    assert D[:3].tolist() == [1.0, 1.0, 1.0] and I[3] == off[R.NONEMPTY + 1] - off[R.NONEMPTY] and D[3] == 0.0
    # the whole mixed list with the flag
    check(kset, *R.recipe_matrices(EMPTY_NAN), *R.recipe_lists()["mixed"], method, EMPTY_NAN)


@METHODS
def test_order_independence(kset, method):
    eI, eD = R.recipe_matrices()
    rows, cols = R.recipe_lists()["mixed"]
    base = check(kset, eI, eD, rows, cols, method)
    assert same_bytes(base, check(kset, eI, eD, rows, cols, method))          # two runs
    p = np.random.default_rng(5).permutation(len(rows))
    got = check(kset, eI, eD, rows[p], cols[p], method)
    assert same_bytes((base[0][p], base[1][p]), got)
    # a pair's slot does not depend on the rest of the list
    sub = check(kset, eI, eD, rows[:37], cols[:37], method)
    assert same_bytes((base[0][:37], base[1][:37]), sub)


def test_outputs_and_empty_list(kset):
    eI, eD = R.recipe_matrices()
    rows, cols = R.recipe_lists()["unit_edges"]
    for method in (SORTED, BITSET):
        check(kset, eI, eD, rows, cols, method, null=("I",))
        check(kset, eI, eD, rows, cols, method, null=("D",))
    from gdist import _lib as L
    assert L.lib.gdist_pairs(kset.ctx.h, kset.h, 0, None, None, AUTO, 0, None, None) == 0
    assert kset.pairs_info() == (-1.0, 0, 0)
    rc, I, D = raw_pairs(kset, [], [])
    assert rc == 0 and untouched(I, D)
    I, D = kset.pairs([], [])
    assert len(I) == len(D) == 0
    I, D = kset.pairs(rows, cols, want_I=False)
    assert I is None and np.array_equal(D.view(np.uint64), R.pairs_ref(eI, eD, rows, cols)[1].view(np.uint64))
    I, D = kset.pairs(rows, cols, want_D=False)
    assert D is None and np.array_equal(I, R.pairs_ref(eI, eD, rows, cols)[0])


def test_einval(kset, ctx):
    """Every refusal of the contract: EINVAL, the outputs still garbage, the
    reason in gdist_last_error."""
    import gdist
    rows, cols = np.array([3, 4, 5], np.int64), np.array([9, 4, 0], np.int64)

    def refused(msg, sets=kset, r=rows, c=cols, **kw):
        rc, I, D = raw_pairs(sets, r, c, **kw)
        assert rc == -1, (msg, rc)
        assert untouched(I, D), msg
        assert msg in last_error(), (msg, last_error())

    refused("npairs outside", npairs=-1)
    refused("npairs outside", npairs=1 << 31)
    refused("null rows or cols", null=("rows",))
    refused("null rows or cols", null=("cols",))
    refused("both outputs null", null=("I", "D"))
    refused("pair index out of range", r=np.array([3, N, 5], np.int64))
    refused("pair index out of range", c=np.array([9, 4, -1], np.int64))
    refused("neither GDIST_UPPER_TRIANGLE nor GDIST_OUT_DEVICE", flags=UPPER_TRIANGLE)
    refused("neither GDIST_UPPER_TRIANGLE nor GDIST_OUT_DEVICE", flags=OUT_DEVICE)
    refused("unknown method", method=3)
    refused("unknown method", method=-1)
    sk = kset.sketches(32)
    refused("pair lists run on kmer sets", sets=sk)
    sk.free()
    b = gdist.KmerSets.from_sequences(CR.recipe_sequences()[:20], 21, gdist.KmerType.DNA, 0, ctx)
    b.build_bitsets()
    b.release_codes()
    refused("this collection holds bitsets only", sets=b, method=SORTED)
    eI, eD = R.recipe_matrices()
    check(b, eI, eD, rows, cols, BITSET)
    b.free()


def test_timing(kset, opts):
    eI, eD = R.recipe_matrices()
    rows, cols = R.recipe_lists()["mixed"]
    opts(time_kernels=1)
    for method in (SORTED, BITSET):
        check(kset, eI, eD, rows, cols, method)
        assert kset.pairs_info()[0] >= 0.0
    opts(time_kernels=0)
    check(kset, eI, eD, rows, cols)
    assert kset.pairs_info()[0] == -1.0


# ---- the tiers of the bitsets ---------------------------------------------
@pytest.fixture(scope="module")
def c4_like():
    from gdist import synth
    n = 1200
    seqs = [bytes(r) for r in synth.genomes(n, 4000, 0.03, 41)]
    off, codes = oracle.pack(seqs, 21, 0, 0)
    return seqs, off, codes


@pytest.mark.parametrize("mode", ["variant", "variant_w64", "two_tier"])
def test_tiers(ctx, opts, c4_like, mode):
    """The dense, rare and variant tiers together count what bitset_matrix
    counts; after release_codes BITSET and AUTO answer the same bytes."""
    import gdist
    seqs, off, codes = c4_like
    n = len(seqs)
    if mode == "two_tier":
        opts(variant=0, rare_t=3)
    else:
        opts(variant=1, rare_t=3, variant_dmin=n // 10, range_summary=1,
             variant_bits=64 if mode == "variant_w64" else None)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    if mode == "two_tier":
        assert sets.variant_info()[:3] == (0, 0, 0)
        assert sets.rare_info()[1] > 0 and sets.rare_info()[2] > 0
    else:
        vk, vw, ve, _ = sets.variant_info()
        assert vk > 1000 and vw > 0 and ve > 0
    eI, eD = refcache.full(off, codes)
    rng = np.random.default_rng(77)
    rows, cols = rng.integers(0, n, 3000), rng.integers(0, n, 3000)
    rows[:3], cols[:3] = (600, 600, 0), (600, n - 1, 600)
    assert (eI[rows, cols] > 0).sum() > 2900                     # related genomes: the tiers all count
    base = check(sets, eI, eD, rows, cols, BITSET)
    sets.release_codes()
    assert same_bytes(base, check(sets, eI, eD, rows, cols, BITSET))
    assert same_bytes(base, check(sets, eI, eD, rows, cols, AUTO))
    rc, I, D = raw_pairs(sets, rows, cols, SORTED)
    assert rc == -1 and untouched(I, D) and "bitsets only" in last_error()
    sets.free()


# ---- large sets: units cut by segment range --------------------------------
def test_large_sets_are_cut(ctx):
    import gdist
    from gdist import synth
    seqs = [bytes(r) for r in synth.genomes(4, 250_000, 0.02, 9)]
    off, codes = oracle.pack(seqs, 21, 0, 0)
    assert np.diff(off).min() > 400_000
    pairs = list(itertools.combinations(range(4), 2)) + [(i, i) for i in range(4)]
    rows, cols = np.array([p[0] for p in pairs]), np.array([p[1] for p in pairs])
    eI, eD = R.pairs_brute(off, codes, rows, cols)
    assert eI[:6].min() > 1000
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    for method in (SORTED, BITSET):
        rc, I, D = raw_pairs(sets, rows, cols, method)
        assert rc == 0, last_error()
        assert np.array_equal(I[:10], eI) and np.array_equal(D[:10].view(np.uint64), eD.view(np.uint64))
        assert np.all(I[10:] == GARBAGE_I) and np.all(D[10:] == GARBAGE_D)
        _, groups, units = sets.pairs_info()
        assert groups == 4
        if method == SORTED:
            assert units > groups, (groups, units)             # the cut path ran
    sets.free()


def test_protein(ctx):
    import gdist
    from gdist import synth
    seqs = [bytes(r) for r in synth.genomes(40, 2000, 0.10, 3, protein=True)]
    off, codes = oracle.pack(seqs, 8, 1, 0)
    eI, eD = refcache.full(off, codes)
    rng = np.random.default_rng(8)
    rows, cols = rng.integers(0, 40, 500), rng.integers(0, 40, 500)
    assert (eI[rows, cols] > 0).sum() > 400
    sets = gdist.KmerSets.from_sequences(seqs, 8, gdist.KmerType.PROT, 0, ctx)
    for method in (SORTED, BITSET):
        check(sets, eI, eD, rows, cols, method)
    sets.free()


def test_append_then_pairs(ctx):
    """Pairs naming appended sets: the segment index is extended, the bitsets rebuilt."""
    import gdist
    seqs = CR.recipe_sequences()
    pick = list(range(40)) + [150, 151, 152, 193]          # the appended five: 150, 151, 152 (duplicates), 193, 100
    order = pick + [100]
    eI, eD = R.recipe_matrices()
    eI, eD = eI[np.ix_(order, order)], eD[np.ix_(order, order)]
    assert eD[5, 40] == 0.0 and eD[5, 41] == 0.0            # set 150 and 151 duplicate set 5
    n0 = len(order) - 5
    sets = gdist.KmerSets.from_sequences([seqs[i] for i in order[:n0]], 21, gdist.KmerType.DNA, 0, ctx)
    rng = np.random.default_rng(4)
    r0, c0 = rng.integers(0, n0, 50), rng.integers(0, n0, 50)
    check(sets, eI, eD, r0, c0, SORTED)                      # builds the segment index
    check(sets, eI, eD, r0, c0, BITSET)                      # builds the bitsets
    assert sets.append([seqs[i] for i in order[n0:]]) == n0
    n = len(order)
    rows = np.concatenate([rng.integers(n0, n, 60), rng.integers(0, n, 60), [n - 1, n - 2]])
    cols = np.concatenate([rng.integers(0, n, 60), rng.integers(n0, n, 60), [n - 1, n - 2]])
    for method in (SORTED, BITSET, AUTO):
        check(sets, eI, eD, rows, cols, method)
    sets.free()


# ---- the methods mirror ----------------------------------------------------
def _genomes():
    from gdist import synth
    from gdist.processors import Genome
    n = 10
    dna = synth.genomes(n, 100_000, 0.05, 1)
    prot = synth.genomes(n, 33_333, 0.10, 1, protein=True)
    ranks = ("superkingdom", "phylum", "class", "order", "family", "genus", "species")
    out = {}
    for i in range(n):
        lin = {r: f"{r}-{i >> (6 - d)}" for d, r in enumerate(ranks)} if i < n - 1 else {}
        gid = f"{83333 + i}.{i + 1}"
        out[gid] = Genome(gid, f"Synthetic genome {i}", [bytes(dna[i]).decode()], [bytes(prot[i]).decode()], lin)
    return out


def test_method_table_whole_list(ctx):
    from gdist import methods as M

    def methods():
        return M.read_method_file(io.StringIO("type\tparms\nprot\tK=8\nkmer\tK=21\n"), ctx)

    genomes = _genomes()
    pairs = list(itertools.combinations(list(genomes), 2))
    rng = np.random.default_rng(3)
    pairs = [pairs[i] for i in rng.permutation(len(pairs))]
    pairs.append(pairs[0])                                   # a repeated pair
    out, stats = io.StringIO(), io.StringIO()
    counts = M.method_table(pairs, methods(), genomes, out, stats=stats, threads=8)
    assert counts == {"pairs": 46, "computed": 46, "reused": 0}
    wout, wstats = io.StringIO(), io.StringIO()
    wcounts = M.method_table(pairs, methods(), genomes, wout, stats=wstats, threads=8, whole_list=True)
    assert wcounts == {"pairs": 46, "computed": 46, "reused": 0, "device_calls": 2}
    assert wout.getvalue() == out.getvalue() and wstats.getvalue() == stats.getvalue()
    assert len(out.getvalue().splitlines()) == 47 and len({l.split("\t")[5] for l in out.getvalue().splitlines()}) > 20
    old = M.load_previous(out.getvalue().splitlines(True), methods())
    keep = dict(list(old.items())[:20])
    pout, pstats = io.StringIO(), io.StringIO()
    pcounts = M.method_table(pairs, methods(), genomes, pout, stats=pstats, previous=keep, threads=8)
    qout, qstats = io.StringIO(), io.StringIO()
    qcounts = M.method_table(pairs, methods(), genomes, qout, stats=qstats, previous=keep, threads=8, whole_list=True)
    assert 0 < pcounts["reused"] < 46
    assert qcounts == dict(pcounts, device_calls=2)
    assert qout.getvalue() == pout.getvalue() == out.getvalue() and qstats.getvalue() == pstats.getvalue()
    ms = methods()
    for m in ms:
        m.pair_distances = None                              # would raise if called with pairs to compute
        m.getDistances = None
    aout = io.StringIO()
    acounts = M.method_table(pairs, ms, genomes, aout, previous=old, threads=8, whole_list=True)
    assert acounts == {"pairs": 46, "computed": 0, "reused": 46, "device_calls": 0}
    assert aout.getvalue() == out.getvalue()
