"""Expected answers of the pairs-within-a-distance query (gdist_within), from a
distance matrix alone: numpy, no call into the library. Shared by
test_within_host.py (CPU) and test_gpu_within.py."""
import numpy as np


def within_ref(D, max_dist, r0=0, c0=0, upper=False, keep_self=False):
    """D[a, b] = d(row r0 + a, column c0 + b). The pairs with d <= max_dist (NaN
    never; with upper only column > row, else the row's own set only with
    keep_self), row ascending then column ascending, as CSR: (rowptr int64[nr + 1],
    cols int64[total] of global columns, d float64[total])."""
    D = np.asarray(D, dtype=np.float64)
    nr, nc = D.shape
    rows = (np.arange(nr, dtype=np.int64) + r0)[:, None]
    cols = (np.arange(nc, dtype=np.int64) + c0)[None, :]
    with np.errstate(invalid="ignore"):
        ok = ~np.isnan(D) & (D <= max_dist)
    if upper:
        ok &= cols > rows
    elif not keep_self:
        ok &= cols != rows
    rowptr = np.zeros(nr + 1, dtype=np.int64)
    rowptr[1:] = np.cumsum(ok.sum(1))
    a, b = np.nonzero(ok)                      # row-major: row ascending, then column
    return rowptr, b.astype(np.int64) + c0, D[a, b]


def within_brute(D, max_dist, r0=0, c0=0, upper=False, keep_self=False):
    """The same answer by plain loops: per row [(global column, d)]."""
    out = []
    for a, row in enumerate(D):
        i, lst = r0 + a, []
        for b, v in enumerate(row):
            j = c0 + b
            if v != v or not v <= max_dist:
                continue
            if upper:
                if j <= i:
                    continue
            elif j == i and not keep_self:
                continue
            lst.append((j, float(v)))
        out.append(lst)
    return out


def as_lists(rowptr, cols, d):
    return [[(int(cols[p]), float(d[p])) for p in range(rowptr[a], rowptr[a + 1])] for a in range(len(rowptr) - 1)]
