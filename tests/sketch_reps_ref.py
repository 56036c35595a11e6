"""Fixtures and references of the sketch representative tests
(test_gpu_sketch_reps.py): the collection, the oracle's full distance matrix a
(width, flags), the sequential loop of gdist_greedy_reps with a tie rank, the
thresholds and the figures gdist_ctx_reps_info must report for a block size.
Nothing here needs a device.

Every case this module hands out is checked on its expected values first: more
than one and fewer than N representatives, at least one row covered only by a
representative of an earlier block and at least one covered only inside its own
block. A test that could pass by covering nothing, or everything, fails here."""
import functools

import numpy as np

import oracle
import sketch_pairs_ref as P
from lifecycle_ref import greedy_ref
from sketch_pairs_ref import ALL_FLAGS, EMPTY_NAN, SKETCH_JACCARD, UPPER_TRIANGLE, bits   # noqa: F401 (the tests' names)

WIDTHS = (64, 65, 1000)
QUANTILES = (0.02, 0.1, 0.3, 0.6)
BLOCK = 32            # the block of the main sweep: the ring kernel's tile
NCOPIES = 3


@functools.lru_cache(maxsize=None)
def collection(width):
    """sketch_pairs_ref.sides(width)[0] (70 signatures, the merge's edge cases
    among random ones) and copies of three non-empty ones of rows 0..63 at
    70, 71, 72: with blocks of 32 every copy sits in another block than its
    original, so t = 0.0 has something to cover across blocks. Returns
    (signatures, the originals' indices)."""
    sigs = list(P.sides(width)[0])
    src = [i for i in (5, 20, 40, 6, 21, 41, 7, 22, 42) if len(sigs[i])][:NCOPIES]
    assert len(src) == NCOPIES and all(i // BLOCK != (len(sigs) + a) // BLOCK for a, i in enumerate(src))
    return tuple(sigs + [sigs[i].copy() for i in src]), tuple(src)


def matrix_of(sigs, width, flags):
    """The oracle's distance of every ordered pair."""
    n = len(sigs)
    D = np.zeros((n, n), np.float64)
    for i in range(n):
        for j in range(n):
            D[i, j] = oracle.sketch_distance(sigs[i], sigs[j], width, flags)[0]
    D.setflags(write=False)
    return D


@functools.lru_cache(maxsize=None)
def expected(width, flags):
    """The oracle's full D of collection(width), computed once and left unchanged."""
    return matrix_of(collection(width)[0], width, flags)


def off_diagonal(D):
    d = D[~np.eye(len(D), dtype=bool)]
    return d[d == d]


@functools.lru_cache(maxsize=None)
def thresholds(width, flags):
    """The 0.02, 0.1, 0.3 and 0.6 quantiles (method "lower") of the off-diagonal
    non-NaN distances: each is a distance that occurs, so the <= tie at the
    threshold is exercised."""
    d = off_diagonal(expected(width, flags))
    ts = tuple(float(np.quantile(d, q, method="lower")) for q in QUANTILES)
    assert all((d == t).any() for t in ts)
    return ts


def greedy(D, t, rank=None):
    """(is_rep int32[N], rep_of int64[N], rep_d float64[N]): lifecycle_ref's
    sequential loop, pass 2 redone under a tie rank (default: the index): the
    least (d, rank) over the representatives with d < 1.0; NaN compares false."""
    n = len(D)
    reps, rep_of, rep_d = greedy_ref(D, t)
    is_rep = np.zeros(n, np.int32)
    is_rep[reps] = 1
    if rank is not None:
        rep_of, rep_d = rep_of.copy(), rep_d.copy()
        for k in range(n):
            if is_rep[k]:
                continue
            cand = [r for r in reps if D[k, r] < 1.0]
            if cand:
                best = min(cand, key=lambda r: (D[k, r], int(rank[r])))
                rep_of[k], rep_d[k] = best, D[k, best]
    return is_rep, np.asarray(rep_of, np.int64), np.asarray(rep_d, np.float64)


def blocks_of(n, block):
    return [(b0, min(n, b0 + block)) for b0 in range(0, n, block)]


def info(is_rep, block, assign):
    """What gdist_ctx_reps_info reports: (row blocks of pass 1, the sum over the
    blocks of rows x representatives chosen before the block, N x R with
    assign else 0, column-list launches: one a block that has representatives
    before it, and one a block in pass 2)."""
    n = len(is_rep)
    bl = blocks_of(n, block)
    before = [int(is_rep[:b0].sum()) for b0, _ in bl]
    cells1 = sum((b1 - b0) * r for (b0, b1), r in zip(bl, before))
    R = int(is_rep.sum())
    return (len(bl), cells1, n * R if assign else 0, sum(1 for r in before if r) + (len(bl) if assign else 0))


def cover_kinds(D, t, is_rep, block):
    """(rows covered only by a representative of an earlier block, rows covered
    only inside their own block)."""
    n = len(D)
    only_earlier = only_inside = 0
    for k in range(n):
        if is_rep[k]:
            continue
        b0 = k // block * block
        earlier = any(is_rep[r] and D[k, r] <= t for r in range(b0))
        inside = any(is_rep[r] and D[k, r] <= t for r in range(b0, k))
        assert earlier or inside
        only_earlier += earlier and not inside
        only_inside += inside and not earlier
    return only_earlier, only_inside


def checked(D, t, block, rank=None):
    """greedy(D, t, rank) after the checks of the module docstring at `block`."""
    is_rep, rep_of, rep_d = greedy(D, t, rank)
    R, n = int(is_rep.sum()), len(D)
    assert 1 < R < n, (t, R)
    only_earlier, only_inside = cover_kinds(D, t, is_rep, block)
    assert only_earlier >= 1 and only_inside >= 1, (t, only_earlier, only_inside)
    for a in (is_rep, rep_of, rep_d):
        a.setflags(write=False)
    return is_rep, rep_of, rep_d


@functools.lru_cache(maxsize=None)
def case(width, flags, t, block=BLOCK):
    """The expected (is_rep, rep_of, rep_d) of collection(width) at threshold t."""
    return checked(expected(width, flags), t, block)


def sweep():
    """(width, flags, t) of the main sweep."""
    return [(w, f, t) for w in WIDTHS for f in ALL_FLAGS for t in thresholds(w, f)]


@functools.lru_cache(maxsize=None)
def tie_ranks(n):
    """name -> rank: a seeded permutation and the reversed index."""
    return {"permuted": np.random.default_rng(31).permutation(n).astype(np.int64),
            "reversed": np.arange(n, dtype=np.int64)[::-1].copy()}


@functools.lru_cache(maxsize=None)
def tie_case(width=64):
    """(flags, t, {name: (is_rep, rep_of, rep_d)}): at width 64 the distances
    are multiples of 1/64, so equal distances to two representatives occur; at
    least one row's winner differs between the two ranks."""
    flags = 0
    t = thresholds(width, flags)[2]        # 0.90625 = 58/64: 24 representatives, 49 rows to assign
    D = expected(width, flags)
    out = {name: greedy(D, t, rank) for name, rank in tie_ranks(len(D)).items()}
    a, b = out["permuted"], out["reversed"]
    assert np.array_equal(a[0], b[0]) and (a[1] != b[1]).any()
    assert np.array_equal(bits(a[2]), bits(b[2]))          # the distance of a tie is one value
    return flags, t, out


@functools.lru_cache(maxsize=None)
def nan_collection(width):
    """collection(width) between two empty signatures. Set 0, empty, is always
    a representative; at t >= 1.0 it covers every non-empty signature (d = 1.0),
    and another empty one too (d = 1.0) unless GDIST_EMPTY_NAN makes that
    distance NaN, which never covers: then every empty signature is a
    representative."""
    empty = np.zeros(0, np.int32)
    return (empty,) + collection(width)[0] + (empty,)


@functools.lru_cache(maxsize=None)
def nan_expected(width, flags):
    D = matrix_of(nan_collection(width), width, flags)
    assert bool(flags & EMPTY_NAN) == bool(np.isnan(D[-1, 0]))
    return D


@functools.lru_cache(maxsize=None)
def built(n=120, length=5000, rate=0.05, seed=11, k=21, width=200):
    """(sequences, D): synth.genomes packed and sketched by the oracle, and the
    oracle's distances of the signatures."""
    from gdist import synth
    seqs = [bytes(r) for r in synth.genomes(n, length, rate, seed)]
    off, codes = oracle.pack(seqs, k, 0, 0)
    sigs = [oracle.sketch(codes[off[i]:off[i + 1]], k, 0, width) for i in range(n)]
    return seqs, matrix_of(sigs, width, 0)
