"""Shared fixture of the cross within / group_stats / histogram tests
(gdist_cross_within, gdist_cross_group_stats, gdist_cross_histogram): numpy
plus the oracle, no call into the library. Used by test_cross_consumers_host.py
(CPU) and test_gpu_cross_consumers.py.

The collections and the expected D are cross_ref.py's: 143 resident subjects,
52 queries, D[NQ, NS] of the oracle with flags 0 and EMPTY_NAN. Two groupings
are defined over the 195 recipe indices and split by SUBJECTS and QUERIES, so
both sides hold some sets without a group. The expected answers come from
within_ref / group_ref / hist_ref on that D, with the labels in the order of
gdist_sets_concat(subjects, queries): the subjects' first, rows from NS on.
"""
import functools

import numpy as np

import cross_ref as X
import group_ref as G
import hist_ref as H
import within_ref as W

NS, NQ, EMPTY_NAN = X.NS, X.NQ, X.EMPTY_NAN
NTYPES = 2


def _recipe_labels():
    g = np.arange(NS + NQ, dtype=np.int32)
    lab = np.stack([g % 4, g % 7]).astype(np.int32)
    lab[:, g % 11 == 0] = -1
    return lab


SLABELS = np.ascontiguousarray(_recipe_labels()[:, X.SUBJECTS])     # [NTYPES, NS]
QLABELS = np.ascontiguousarray(_recipe_labels()[:, X.QUERIES])      # [NTYPES, NQ]
LABELS = np.ascontiguousarray(np.concatenate([SLABELS, QLABELS], axis=1))   # of concat(subjects, queries)
for _a in (SLABELS, QLABELS, LABELS):
    _a.setflags(write=False)

# the reference's 50 buckets over [0, 1] (TaxCheckProcessor.java:93): edges i / 50
EDGES50 = np.array([i / 50 for i in range(51)], dtype=np.float64)
EDGES50.setflags(write=False)


def expected_d(flags=0):
    return X.expected(flags)[1]


def within_expected(max_dist, flags=0, rows=None, cols=None):
    """(rowptr, cols, d) of query rows x subject cols; the columns are subject indices."""
    r0, r1 = rows or (0, NQ)
    c0, c1 = cols or (0, NS)
    return W.within_ref(expected_d(flags)[r0:r1, c0:c1], max_dist, r0, c0, upper=False, keep_self=True)


def group_expected(flags=0, rows=None, cols=None, types=None):
    r0, r1 = rows or (0, NQ)
    c0, c1 = cols or (0, NS)
    lab = LABELS if types is None else LABELS[types]
    return G.group_ref(expected_d(flags)[r0:r1, c0:c1], lab, NS + r0, c0, upper=False)


def hist_expected(edges, flags=0, rows=None, cols=None, labelled=True):
    r0, r1 = rows or (0, NQ)
    c0, c1 = cols or (0, NS)
    return H.hist_ref(expected_d(flags)[r0:r1, c0:c1], edges, LABELS if labelled else None, NS + r0, c0,
                      upper=False)


@functools.lru_cache(maxsize=None)
def ulp_edges():
    """Edges one ulp apart around a distance that occurs (the median of the
    d < 1.0 cells), an edge at exactly 1.0 and the two infinities."""
    D = expected_d(0)
    v = np.sort(D[D < 1.0])
    x = v[len(v) // 2]
    e = np.array([-np.inf, 0.0, np.nextafter(x, 0.0), x, np.nextafter(x, 1.0), 1.0, np.inf], dtype=np.float64)
    assert np.all(np.diff(e) > 0)
    e.setflags(write=False)
    return e


def numbers():
    """Everything check_fixture pins, as computed now."""
    out = {}
    rp, _, _ = within_expected(0.9)
    per = np.diff(rp)
    out["w09"] = (int((per == 0).sum()), int((per >= 10).sum()), int(rp[-1]))
    out["w00"] = int(within_expected(0.0)[0][-1])
    out["w10"] = int(within_expected(1.0)[0][-1])
    out["w10_nan"] = int(within_expected(1.0, EMPTY_NAN)[0][-1])
    g = group_expected(0)
    out["group"] = [(t["bad"], [(s["n"], s["ones"], s["nans"]) for s in t["sides"]]) for t in g]
    g = group_expected(EMPTY_NAN)
    out["group_nan"] = [(t["bad"], [(s["n"], s["ones"], s["nans"]) for s in t["sides"]]) for t in g]
    c, n, b = hist_expected(EDGES50, EMPTY_NAN)
    assert not c[:, 0].any()                               # nothing below the edge at 0.0
    out["hist_nonempty"] = [int((row[1:51] > 0).sum()) for row in c]    # bucket b: [(b - 1) / 50, b / 50)
    out["hist_ones"] = [int(row[51]) for row in c]                      # bucket 51: d >= 1.0
    out["hist_nans"] = n.tolist()
    c, n, _ = hist_expected(EDGES50, EMPTY_NAN, labelled=False)
    out["hist_all"] = (int((c[0][1:51] > 0).sum()), int(c[0][51]), int(n[0]))
    c, _, _ = hist_expected(ulp_edges(), 0, labelled=False)
    out["hist_ulp"] = c[0].tolist()
    return out


def check_fixture():
    """The conditions the cross consumer tests rely on; a fixture that stopped
    exercising them fails here instead of passing quietly."""
    X.check_fixture()
    assert SLABELS.shape == (NTYPES, NS) and QLABELS.shape == (NTYPES, NQ)
    # both sides hold sets without a group
    assert int((SLABELS[0] < 0).sum()) == 13 and int((QLABELS[0] < 0).sum()) == 5
    assert np.array_equal(SLABELS < 0, np.stack([SLABELS[0] < 0] * 2))
    n = numbers()
    # within 0.9: 20 query rows have no neighbour, 30 have at least 10; the
    # total is neither 0 nor every cell
    assert n["w09"] == W09 and 0 < n["w09"][2] < NQ * NS
    assert n["w09"][:2] == (20, 30)
    assert n["w00"] == 3                                   # the three duplicates
    assert n["w10"] == NQ * NS and n["w10_nan"] == NQ * NS - 1
    # in every grouping both sides hold summarised values and ones; bad > 0
    assert n["group"] == GROUP
    for bad, sides in n["group"]:
        assert bad > 0 and all(s[0] > 0 and s[1] > 0 and s[2] == 0 for s in sides)
    # EMPTY_NAN: exactly one NaN cell, and it lands in a series
    assert n["group_nan"] == GROUP_NAN
    assert [sum(s[2] for s in sides) for _, sides in n["group_nan"]] == [1, 1]
    assert n["hist_nans"] == HIST_NANS and [sum(HIST_NANS[2 * t:2 * t + 2]) for t in range(NTYPES)] == [1, 1]
    # the 50 buckets: at least 5 non-empty below 1.0 in every series, and the
    # edge at 1.0 separates exactly the ones
    assert n["hist_nonempty"] == HIST_NONEMPTY and min(HIST_NONEMPTY) >= 5
    ones = [s[1] for _, sides in n["group_nan"] for s in sides]
    assert n["hist_ones"] == ones
    assert n["hist_all"] == HIST_ALL and HIST_ALL[0] >= 5 and HIST_ALL[2] == 1
    assert HIST_ALL[1] == NQ * NS - 3960 - 1               # d == 1.0 cells (cross_ref pins 3960 below 1.0)
    # the ulp-apart edges: the distance they surround is in its own bucket
    # (buckets: d < -inf, [-inf, 0), [0, x-), [x-, x), [x, x+), [x+, 1), [1, inf), d >= inf)
    assert n["hist_ulp"] == HIST_ULP and HIST_ULP[4] > 0 and HIST_ULP[3] == 0
    assert HIST_ULP[0] == HIST_ULP[1] == HIST_ULP[7] == 0 and sum(HIST_ULP) == NQ * NS


# the numbers of numbers() on this fixture
W09 = (20, 30, 1645)                       # rows with no pair, rows with >= 10, pairs within 0.9
# per grouping (bad, [in, out] as (n, ones, nans)), flags 0 and EMPTY_NAN
GROUP = [(1326, [(817, 711, 0), (2453, 2129, 0)]), (1326, [(465, 403, 0), (2805, 2437, 0)])]
GROUP_NAN = [(1326, [(817, 711, 0), (2453, 2128, 1)]), (1326, [(465, 403, 0), (2805, 2436, 1)])]
HIST_NANS = [0, 1, 0, 1]                   # per series, EMPTY_NAN
HIST_NONEMPTY = [34, 44, 33, 43]           # per series: non-empty buckets of the 50 below 1.0
HIST_ALL = (45, 3475, 1)                   # one series: non-empty buckets, d == 1.0 cells, NaN cells
HIST_ULP = [0, 0, 1978, 0, 3, 1979, 3476, 0]
