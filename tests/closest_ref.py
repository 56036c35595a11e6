"""Expected answers of the exact nearest-neighbour query (gdist_closest), from
a distance matrix alone: numpy, no call into the library. Shared by
test_closest_host.py (CPU) and test_gpu_closest.py.

Also the shared fixture recipe of those tests: 195 DNA sequences (150 related,
three exact duplicates, 40 unrelated, two without a 21-mer) packed by the
oracle, with its distance matrix, computed once per process.
"""
import functools

import numpy as np


def closest_ref(D, n, max_dist, r0=0, c0=0, keep_self=False):
    """D[a, b] = d(row r0 + a, column c0 + b). For every row the columns with
    d <= max_dist (NaN never, the row's own set unless keep_self), ordered by
    (d, column), the first n: (idx[nr, n] int64 of global columns, d[nr, n]
    float64, count[nr] int32); unused slots -1 / 1.0."""
    D = np.asarray(D, dtype=np.float64)
    nr, nc = D.shape
    idx = np.full((nr, n), -1, dtype=np.int64)
    d = np.ones((nr, n), dtype=np.float64)
    cnt = np.zeros(nr, dtype=np.int32)
    cols = np.arange(nc, dtype=np.int64) + c0
    for a in range(nr):
        row = D[a]
        with np.errstate(invalid="ignore"):
            ok = ~np.isnan(row) & (row <= max_dist)
        if not keep_self:
            ok &= cols != r0 + a
        cand = np.flatnonzero(ok)
        order = np.lexsort((cols[cand], row[cand]))      # by d, then by column
        take = cand[order][:n]
        cnt[a] = len(take)
        idx[a, :len(take)] = cols[take]
        d[a, :len(take)] = row[take]
    return idx, d, cnt


def closest_brute(D, n, max_dist, r0=0, c0=0, keep_self=False):
    """The same answer by plain loops and a Python sort of (d, column) tuples."""
    out = []
    for a, row in enumerate(D):
        c = []
        for b, v in enumerate(row):
            j = c0 + b
            if v != v or not v <= max_dist or (j == r0 + a and not keep_self):
                continue
            c.append((float(v), j))
        c.sort()
        out.append([(j, v) for v, j in c[:n]])
    return out


def as_lists(idx, d, cnt):
    return [[(int(idx[a, r]), float(d[a, r])) for r in range(cnt[a])] for a in range(len(cnt))]


def recipe_sequences():
    from gdist import synth
    rel = [bytes(r) for r in synth.genomes(150, 3000, 0.08, 41)]
    dup = [rel[5], rel[5], rel[77]]
    unrel = [bytes(synth.genomes(1, 3000, 0.0, 100 + i)[0]) for i in range(40)]
    return rel + dup + unrel + [b"", b"ACGTACGT"]


@functools.lru_cache(maxsize=None)
def recipe(flags=0):
    """(sequences, oracle offsets, oracle codes, oracle D with `flags`) of the
    recipe, DNA, k = 21, default pack flags; N = 195. Read-only."""
    import oracle
    seqs = recipe_sequences()
    off, codes = oracle.pack(seqs, 21, 0, 0)
    n = len(seqs)
    _, D = oracle.matrix(off, codes, 0, n, 0, n, flags=flags)
    D.setflags(write=False)
    return seqs, off, codes, D
