"""Expected answers of the distance histogram (gdist_histogram), from a
distance matrix, bucket edges and labels alone: numpy, no call into the
library. Shared by test_hist_host.py (CPU) and test_gpu_hist.py.

A non-NaN d goes to bucket numpy.searchsorted(edges, d, side="right"), the
number of edges <= d; NaN is counted apart and is in no bucket. Without labels
there is one series of every pair; with labels [T, N] the pairs are split as
GroupTypeSpec.java:77-95 splits them: a label < 0 on either set is a bad pair
and nothing else, equal labels are series 2 t (in-group), others series 2 t + 1.
"""
import numpy as np


def _series(D, labels, r0, c0, upper):
    """(bad counts [T], one boolean mask over D per series)."""
    nr, nc = D.shape
    rows, cols = np.arange(nr) + r0, np.arange(nc) + c0
    take = cols[None, :] > rows[:, None] if upper else np.ones((nr, nc), dtype=bool)
    if labels is None:
        return [], [take]
    bad, masks = [], []
    for lab in np.atleast_2d(np.asarray(labels, dtype=np.int64)):
        la, lb = lab[rows][:, None], lab[cols][None, :]
        isbad = take & ((la < 0) | (lb < 0))
        ok = take & ~isbad
        same = ok & (la == lb)
        bad.append(int(isbad.sum()))
        masks += [same, ok & ~same]
    return bad, masks


def hist_ref(D, edges, labels=None, r0=0, c0=0, upper=True):
    """D[a, b] = d(set r0 + a, set c0 + b); labels None, [N] or [T, N] over the
    whole collection. upper: only the pairs with global column > global row.
    Returns (counts int64 [S, E + 1], nans int64 [S], bad int64 [T])."""
    D = np.asarray(D, dtype=np.float64)
    edges = np.asarray(edges, dtype=np.float64)
    bad, masks = _series(D, labels, r0, c0, upper)
    counts = np.zeros((len(masks), len(edges) + 1), dtype=np.int64)
    nans = np.zeros(len(masks), dtype=np.int64)
    for s, mask in enumerate(masks):
        v = D[mask]
        isnan = np.isnan(v)
        nans[s] = isnan.sum()
        counts[s] = np.bincount(np.searchsorted(edges, v[~isnan], side="right"), minlength=len(edges) + 1)
    return counts, nans, np.array(bad, dtype=np.int64)


def hist_brute(D, edges, labels=None, r0=0, c0=0, upper=True):
    """The same answer by plain loops: the bucket is the count of edges <= d."""
    edges = [float(e) for e in edges]
    labs = [] if labels is None else [[int(x) for x in lab] for lab in np.atleast_2d(np.asarray(labels))]
    S = 2 * len(labs) if labs else 1
    counts = [[0] * (len(edges) + 1) for _ in range(S)]
    nans, bad = [0] * S, [0] * len(labs)

    def add(s, d):
        if d != d:
            nans[s] += 1
        else:
            counts[s][sum(1 for e in edges if e <= d)] += 1
    for a, row in enumerate(D):
        for b, d in enumerate(row):
            i, j = r0 + a, c0 + b
            if upper and j <= i:
                continue
            if not labs:
                add(0, float(d))
            for t, lab in enumerate(labs):
                if lab[i] < 0 or lab[j] < 0:
                    bad[t] += 1
                else:
                    add(2 * t + (0 if lab[i] == lab[j] else 1), float(d))
    return (np.array(counts, dtype=np.int64).reshape(S, len(edges) + 1), np.array(nans, dtype=np.int64),
            np.array(bad, dtype=np.int64))


def pattern_edges(n, lo=0.0, hi=1.0):
    """n doubles at evenly spaced bit patterns strictly between lo's and hi's (0 <= lo < hi)."""
    a, b = (int(np.float64(x).view(np.uint64)) for x in (lo, hi))
    pats = sorted({a + (i * (b - a)) // (n + 1) for i in range(1, n + 1)} - {a, b})
    return np.array(pats, dtype=np.uint64).view(np.float64)


def rank_of(q, n):
    """k of the order statistic x_k that quantile q of n values names."""
    import math
    return max(1, min(n, int(math.ceil(q * n))))
