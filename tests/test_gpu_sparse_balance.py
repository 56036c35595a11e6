"""Sparse tile chunks by modelled cost (option sparse_balance: 1 equal costs,
2 costs tapering along a tile's chunks, the default): bounds from the
per-granule products profile, three quarters as many chunks for the diagonal
tiles (their own bounds table and partial base per tile), and the workgroup ->
(tile, chunk) map in descending cost. Every setting is bit-exact
against the oracle, I and D, over the whole upper triangle, a row-trimmed
block, a non-upper rectangle (diagonal tiles mirrored) and the whole square,
on a collection of 300 sets (2 x 128 + 44: a partial last block)."""
import re

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, LENGTH = 300, 20000


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


_DATA = {}


def collection(name):
    """base: the sparse parity sweep's collection (300 x 20 kbp, p 0.003, seed
    105). skewed: the same with 60 more substitutions a genome packed into
    [0.6 L, 0.7 L), so that the sparse words of that tenth of the locus order
    have several times the holders (and products) of the rest. With the
    oracle's whole N x N matrices, computed once."""
    if name not in _DATA:
        from gdist import synth
        g = synth.genomes(N, LENGTH, 0.003, 105)
        if name == "skewed":
            g = g.copy()
            rng = np.random.RandomState(20250)
            comp = np.zeros(256, np.uint8)
            comp[list(b"ACGT")] = list(b"CGTA")
            for r in range(N):
                pos = rng.randint(int(0.6 * LENGTH), int(0.7 * LENGTH), 60)
                g[r, pos] = comp[g[r, pos]]
        seqs = [bytes(r) for r in g]
        off, codes = oracle.pack(seqs, 21, 0, 0)
        eI, eD = oracle.matrix(off, codes, 0, N, 0, N, flags=0, nthreads=8)
        _DATA[name] = (seqs, eI, eD)
    return _DATA[name]


REGIONS = [(0, N, 0, N, True),            # the whole upper triangle
           (100, 250, 0, N, True),        # rows trimmed at both ends of the block range
           (37, 211, 5, 290, False),      # a rectangle: diagonal tiles row-trimmed or mirrored
           (0, N, 0, N, False)]           # the whole square: every diagonal tile mirrored

ALL = {"sparse_zmax": 100000}
MODES = {
    "balanced_default": dict(ALL),
    "equal_default": dict(ALL, sparse_balance=0),
    # equal costs without the taper
    "flat_default": dict(ALL, sparse_balance=1),
    "flat_c3": dict(ALL, sparse_balance=1, sparse_chunks=3),
    "flat_c7": dict(ALL, sparse_balance=1, sparse_chunks=7),
    "flat_c37": dict(ALL, sparse_balance=1, sparse_chunks=37),
    "flat_atomic": dict(ALL, sparse_balance=1, sparse_part_budget=0, sparse_chunks=5),
    # 1, 2 and 3 chunks: the diagonal tiles keep the same count; 7 and 37
    # leave their table a remainder (ceil(3 n / 4) = 6 and 28 chunks)
    "balanced_c1": dict(ALL, sparse_chunks=1),
    "balanced_c2": dict(ALL, sparse_chunks=2),
    "balanced_c3": dict(ALL, sparse_chunks=3),
    "balanced_c7": dict(ALL, sparse_chunks=7),
    "balanced_c37": dict(ALL, sparse_chunks=37),
    "equal_c7": dict(ALL, sparse_balance=0, sparse_chunks=7),
    "equal_c37": dict(ALL, sparse_balance=0, sparse_chunks=37),
    # chunks flush with atomics: the constant part once a tile, by its chunk 0
    "balanced_atomic": dict(ALL, sparse_part_budget=0, sparse_chunks=5),
    "balanced_atomic_c2": dict(ALL, sparse_part_budget=0, sparse_chunks=2),
    "equal_atomic": dict(ALL, sparse_balance=0, sparse_part_budget=0, sparse_chunks=5),
    # the XCD-mapped launch keeps one table, a uniform count and its own order
    "balanced_xcd": dict(ALL, sparse_xcd=1, sparse_chunks=13),
    "balanced_mt1": dict(ALL, sparse_mt=1, sparse_chunks=7),
    # dense words folded into the first chunks of every tile: a diagonal tile
    # keeps at least a chunk per slab
    "balanced_slabs_c2": {"sparse_zmax": 12, "sparse_fold": 100000, "sparse_chunks": 2},
    "balanced_slabs_c7": {"sparse_zmax": 12, "sparse_fold": 100000, "sparse_chunks": 7},
    "balanced_slabs_atomic": {"sparse_zmax": 12, "sparse_fold": 100000, "sparse_chunks": 3, "sparse_part_budget": 0},
    # the automatic choice of sparse words, rare tier and group tier included
    "balanced_auto_c7": {"sparse_chunks": 7},
}
CASES = [("base", m) for m in MODES] + [("skewed", m) for m in ("balanced_default", "balanced_c3", "balanced_c7",
                                                                "balanced_c37", "equal_c7", "balanced_atomic",
                                                                "flat_c7", "flat_c37", "flat_atomic",
                                                                "balanced_slabs_c7", "balanced_auto_c7")]


def check_regions(sets, eI, eD, tag):
    import gdist
    for (r0, r1, c0, c1, up) in REGIONS:
        I, D = sets.matrix((r0, r1), (c0, c1), upper=up, method=gdist.METHOD_BITSET)
        xI, xD = eI[r0:r1, c0:c1], eD[r0:r1, c0:c1]
        if up:
            mask = np.fromfunction(lambda a, b: (c0 + b) > (r0 + a), (r1 - r0, c1 - c0))
            I, D, xI, xD = I[mask], D[mask], xI[mask], xD[mask]
        assert np.array_equal(I, xI), (tag, r0, r1, c0, c1, up)
        assert bits_equal(D, xD), (tag, r0, r1, c0, c1, up)


@pytest.mark.parametrize("data,mode", CASES, ids=[f"{d}-{m}" for d, m in CASES])
def test_balanced_chunks_exact(ctx, opts, data, mode):
    import gdist
    seqs, eI, eD = collection(data)
    opts(**MODES[mode])
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    ws, wd, ent = sets.sparse_info()
    assert ws > 0 and ent > 0
    if "slabs" in mode:
        assert wd > 0
    elif "auto" not in mode:
        assert wd == 0
    check_regions(sets, eI, eD, (data, mode))


PLAN_LINE = re.compile(r"sparse chunks (balanced|balanced \(tapered\)|at equal counts): (\d+) a tile \((\d+) on the diagonal\), (\d+) workgroups "
                       r"(heaviest first|tile-major); modelled cost max / mean ([0-9.]+) \(chunk (\d+)\), "
                       r"at equal counts ([0-9.]+) \(chunk (\d+)\); (\d+) of (\d+) bounds differ")


def plan_of(ctx, opts, capfd, sets, **o):
    """The plan line option trace prints when the whole triangle's plan is built."""
    import gdist
    opts(trace=1, **o)
    capfd.readouterr()
    sets.matrix(upper=True, method=gdist.METHOD_BITSET)
    err = capfd.readouterr().err
    opts(trace=None)
    m = [PLAN_LINE.search(line) for line in err.splitlines()]
    m = [x for x in m if x]
    assert m, err[-2000:]
    kind, nch, nd, wgs, order, sk, at, sk_eq, at_eq, moved, nb = m[-1].groups()
    return dict(kind=kind, nch=int(nch), nd=int(nd), wgs=int(wgs), order=order, skew=float(sk), at=int(at),
                skew_eq=float(sk_eq), at_eq=int(at_eq), moved=int(moved), nb=int(nb))


def test_skew_moves_the_bounds(ctx, opts, capfd):
    """On the skewed collection the table of equal costs (sparse_balance 1)
    differs from the equal-count one and its modelled max / mean chunk cost is
    lower; the diagonal tiles get ceil(3 n / 4) chunks and the workgroups go
    heaviest first. The default (tapered) plan has the same counts and order
    and its own bounds. Option sparse_balance 0 gives the equal-count table,
    one count, and tile-major order."""
    import gdist
    seqs, eI, eD = collection("skewed")
    opts(sparse_zmax=100000, sparse_chunks=7)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    bal = plan_of(ctx, opts, capfd, sets, sparse_balance=1)
    # 300 sets: 3 blocks, 6 tiles of the upper triangle, 3 of them diagonal
    assert bal["kind"] == "balanced" and bal["nch"] == 7 and bal["nd"] == 6 and bal["wgs"] == 3 * 7 + 3 * 6, bal
    assert bal["order"] == "heaviest first" and bal["nb"] == 8, bal
    assert bal["moved"] > 0 and bal["skew"] < bal["skew_eq"], bal
    tap = plan_of(ctx, opts, capfd, sets, sparse_balance=None)
    assert tap["kind"] == "balanced (tapered)" and tap["nch"] == 7 and tap["nd"] == 6 and tap["wgs"] == 39, tap
    assert tap["order"] == "heaviest first" and tap["moved"] > 0, tap
    eq = plan_of(ctx, opts, capfd, sets, sparse_balance=0)
    assert eq["kind"] == "at equal counts" and eq["nch"] == 7 and eq["nd"] == 7 and eq["wgs"] == 6 * 7, eq
    assert eq["order"] == "tile-major" and eq["moved"] == 0 and eq["skew"] == eq["skew_eq"], eq
    assert eq["skew_eq"] == bal["skew_eq"] and eq["at_eq"] == bal["at_eq"], (eq, bal)
    assert bal["skew"] < eq["skew"], (bal, eq)


def test_balanced_replayed_steps_poisoned(ctx, opts):
    """Repeated device-output calls over one region with the balanced plan
    (the first builds the plan, the second is captured, the rest replay the
    graph) into outputs poisoned before every call: every call equals the
    oracle over the region's upper triangle."""
    import gdist
    seqs, eI, eD = collection("skewed")
    opts(sparse_zmax=100000, sparse_chunks=7)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    for (r0, r1) in [(0, N), (100, 250)]:
        nr = r1 - r0
        mask = np.fromfunction(lambda a, b: b > (r0 + a), (nr, N))
        dI, dD = ctx.alloc(nr * N * 4), ctx.alloc(nr * N * 8)
        pI, pD = np.full(nr * N, -7, np.int32), np.full(nr * N, 42.5)
        for call in range(4):
            dI.from_host(pI)
            dD.from_host(pD)
            sets.matrix_device(dI.ptr, dD.ptr, N, (r0, r1), (0, N), upper=True, method=gdist.METHOD_BITSET)
            I = dI.to_host(np.int32).reshape(nr, N)
            D = dD.to_host(np.float64).reshape(nr, N)
            assert np.array_equal(I[mask], eI[r0:r1][mask]), (r0, call)
            assert bits_equal(D[mask], eD[r0:r1][mask]), (r0, call)
        dI.free()
        dD.free()
