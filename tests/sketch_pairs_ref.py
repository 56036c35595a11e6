"""Fixtures and references of the sketch pair-list tests
(test_gpu_sketch_pairs.py, test_sketch_pairs_host.py): the edge-case signatures
of the sketch cross tests restated, the oracle's expected rectangle computed
once a (width, flags) and shared, the list shapes, the unit count of a list and
the row-query reductions in plain Python. Nothing here needs a device."""
import functools

import numpy as np

import oracle

UPPER_TRIANGLE, OUT_DEVICE, EMPTY_NAN, SKETCH_JACCARD, KEEP_SELF = 0x100, 0x200, 0x400, 0x800, 0x1000
ALL_FLAGS = (0, SKETCH_JACCARD, EMPTY_NAN, SKETCH_JACCARD | EMPTY_NAN)
INT_MIN, INT_MAX = -(1 << 31), (1 << 31) - 1
NSUBJ, NQRY = 70, 33   # 70 columns: more than a unit of 64 pairs a row
UNIT = 64              # pairs of one row a unit holds at most (gdist.h)
WIDTHS = (1, 64, 65, 130, 1000)


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


@functools.lru_cache(maxsize=None)
def sides(width):
    """(subjects, queries): NSUBJ and NQRY signatures, the edges among random
    ones; every third subject long against short queries (na < 64 < nb for the
    wide widths). Query 0 is a full signature, query 8 the empty one."""
    rng = np.random.default_rng(1000 + width)
    subj = edge_sigs(rng, width)
    qry = edge_sigs(rng, width)
    while len(subj) < NSUBJ:
        n = int(rng.integers(0, width + 1))
        subj.append(random_sig(rng, width if len(subj) % 3 == 0 else n, -2 * width, 2 * width + 8))
    while len(qry) < NQRY:
        n = int(rng.integers(0, min(width, 40) + 1))
        qry.append(random_sig(rng, width if len(qry) % 4 == 0 else n, -2 * width, 2 * width + 8))
    order = rng.permutation(NSUBJ)
    subj = [subj[i] for i in order]
    qry = qry[:NQRY]
    qry[0], qry[8] = qry[8], qry[0]
    return subj, qry


def rectangle(qry, subj, width, flags):
    """The oracle's (common, D) of every (query, subject) cell."""
    I = np.zeros((len(qry), len(subj)), np.int32)
    D = np.zeros((len(qry), len(subj)), np.float64)
    for a, q in enumerate(qry):
        for b, s in enumerate(subj):
            D[a, b], I[a, b] = oracle.sketch_distance(q, s, width, flags)
    return I, D


@functools.lru_cache(maxsize=None)
def expected(width, flags):
    """The oracle's rectangle of sides(width), computed once and left unchanged."""
    subj, qry = sides(width)
    I, D = rectangle(qry, subj, width, flags)
    I.setflags(write=False)
    D.setflags(write=False)
    return I, D


def one_row(row, n):
    """n pairs of one row; the columns repeat past NSUBJ."""
    return np.full(n, row, np.int64), np.arange(n, dtype=np.int64) % NSUBJ


@functools.lru_cache(maxsize=None)
def lists():
    """name -> (rows into the queries, cols into the subjects)."""
    rng = np.random.default_rng(2024)
    rr, cc = np.divmod(rng.permutation(NQRY * NSUBJ).astype(np.int64), NSUBJ)
    out = {"rectangle": (rr, cc)}                                        # (a) every cell, shuffled
    for n in (63, 64, 65, 200):                                          # (b) around the unit cap
        out[f"row_{n}"] = one_row(0, n)
    out["singles"] = (np.arange(NQRY, dtype=np.int64), (np.arange(NQRY, dtype=np.int64) * 7 + 3) % NSUBJ)   # (c)
    out["repeat"] = (np.full(5, 4, np.int64), np.full(5, 9, np.int64))   # (d)
    out["single"] = (np.array([12], np.int64), np.array([69], np.int64))  # (e)
    return out


def runs_and_singles():
    """List (b) on four rows of its own plus list (c) in one list."""
    parts = [one_row(r, n) for r, n in ((0, 63), (1, 64), (2, 65), (3, 200))] + [lists()["singles"]]
    return np.concatenate([p[0] for p in parts]), np.concatenate([p[1] for p in parts])


def unit_count(rows):
    """sum over the distinct rows of ceil(run / UNIT)."""
    counts = np.unique(np.asarray(rows), return_counts=True)[1]
    return int(((counts + UNIT - 1) // UNIT).sum())


def wide_sides():
    """Width 20,000: five subjects by four queries, one query a subject's copy."""
    rng = np.random.default_rng(7)
    subj = [random_sig(rng, n, -40000, 40000) for n in (20000, 20000, 9000, 63, 0)]
    qry = [random_sig(rng, n, -40000, 40000) for n in (20000, 17, 12000, 20000)]
    qry[3] = subj[1].copy()
    return subj, qry


# ---- gdist_row_query's reductions, one distance at a time ---------------------
def any_le(ds, t):
    for d in ds:
        if d == d and d <= t:
            return True
    return False


def argmin(ds):
    """(position, distance) of the smallest distance below 1.0, the lowest
    position among equals; (-1, 1.0) when there is none. NaN never qualifies."""
    best, bd = -1, 1.0
    for i, d in enumerate(ds):
        if d == d and d < bd:
            best, bd = i, float(d)
    return best, bd
