"""Expected answers of the pair-list call (gdist_pairs) from the oracle's
matrices alone: numpy, no call into the library. Shared by test_pairs_host.py
(CPU), test_gpu_pairs.py and test_gpu_pairs_jni.py, with the pair lists those
tests run over the closest_ref recipe (N = 195)."""
import functools

import numpy as np

import closest_ref as CR

N = 195
NONEMPTY, EMPTY_A, EMPTY_B = 7, 193, 194     # a non-empty set and the recipe's two empty ones


def pairs_ref(I, D, rows, cols):
    """I, D: the oracle's whole matrices (diagonal: the set sizes and their
    distance). The pair list's answer is their cells (rows[p], cols[p])."""
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    return np.ascontiguousarray(I[rows, cols], np.int32), np.ascontiguousarray(D[rows, cols], np.float64)


def pairs_brute(off, codes, rows, cols, flags=0):
    """The same answer pair by pair: oracle.intersect and oracle.distance."""
    import oracle
    I, D = [], []
    for i, j in zip(rows, cols):
        a, b = codes[off[i]:off[i + 1]], codes[off[j]:off[j + 1]]
        inter = len(a) if i == j else oracle.intersect(a, b)
        I.append(inter)
        D.append(oracle.distance(inter, len(a), len(b), flags))
    return np.array(I, np.int32), np.array(D, np.float64)


@functools.lru_cache(maxsize=None)
def recipe_matrices(flags=0):
    """(I, D) of the closest_ref recipe with `flags` (0 or GDIST_EMPTY_NAN),
    the diagonal set to the set sizes and their distance. Read-only."""
    import oracle
    _, off, codes, _ = CR.recipe()
    I, D = oracle.matrix(off, codes, 0, N, 0, N, flags=flags)
    sizes = np.diff(off)
    idx = np.arange(N)
    I[idx, idx] = sizes
    D[idx, idx] = [oracle.distance(int(s), int(s), int(s), flags) for s in sizes]
    I.setflags(write=False)
    D.setflags(write=False)
    return I, D


@functools.lru_cache(maxsize=None)
def recipe_lists():
    """name -> (rows, cols) int64 arrays over the recipe's 195 sets."""
    rng = np.random.default_rng(20261020)
    out = {}
    # every row at most once, shuffled
    r = rng.permutation(N)
    out["singletons"] = (r, rng.integers(0, N, N))
    # row 7 against every column (itself included) among pairs of other rows
    r = np.concatenate([np.full(N, NONEMPTY), rng.integers(8, N, 60)])
    c = np.concatenate([np.arange(N), rng.integers(0, N, 60)])
    p = rng.permutation(len(r))
    out["long_group"] = (r[p], c[p])
    # rows with exactly 1, 63, 64, 65, 128 and 129 listed columns
    r, c = [], []
    for row, k in zip((3, 20, 41, 88, 150, 170), (1, 63, 64, 65, 128, 129)):
        r += [row] * k
        c += rng.choice(N, k, replace=False).tolist()
    p = rng.permutation(len(r))
    out["unit_edges"] = (np.array(r)[p], np.array(c)[p])
    # 2,000 pairs with replacement, with repeats, self pairs and the two empty sets
    r, c = rng.integers(0, N, 2000), rng.integers(0, N, 2000)
    r[:6] = (12, 12, NONEMPTY, EMPTY_A, EMPTY_A, EMPTY_B)
    c[:6] = (90, 90, NONEMPTY, EMPTY_A, EMPTY_B, EMPTY_A)
    p = rng.permutation(2000)
    out["mixed"] = (r[p], c[p])
    for v in out.values():
        for a in v:
            a.setflags(write=False)
    return {k: (np.asarray(a, np.int64), np.asarray(b, np.int64)) for k, (a, b) in out.items()}
