"""Shared fixtures of the cross pair-list tests (gdist_cross_pairs): numpy plus
the oracle, no call into the library. Used by test_cross_pairs_host.py (CPU)
and test_gpu_cross_pairs.py.

Recipe lists. cross_ref.py's split of the 195-sequence recipe (143 subjects,
52 queries, nseg = 3, an empty query, a subject without a 21-mer) with pair
lists whose rows index the queries and whose columns index the subjects; the
expected answers are the cells of cross_ref.expected(flags).

Foreign cut. Synthetic codes (KmerSets.from_codes, PROT k = 8) whose queries
are cut by splitters that were never theirs: a query of 20,000 codes inside one
window of width 2^40, so that at least one of its segments is longer than the
4,096 keys the join stages at a time, a query below every splitter, a query
above every splitter that holds the all-ones code, and the empty query.
"""
import functools

import numpy as np

import cross_ref as X

NS, NQ = X.NS, X.NQ
EMPTY_NAN = X.EMPTY_NAN
EMPTY_Q, KMERLESS_S = NQ - 1, NS - 1      # the empty query, the subject without a 21-mer
LONG_ROW = 7                              # long_group's query
REPEATED = (12, 90)
EDGE_ROWS = {3: 1, 11: 63, 20: 64, 29: 65, 40: 128, 47: 129}
UNIT, UNIT_CODES_MIN = 64, 1 << 14        # pairs a chunk holds at most; the smallest code budget of a unit
STAGE = 4096                              # keys of a query the join stages at a time


def duplicate_pair():
    """(query, subject) of the first exact duplicate: d = 0.0."""
    q, s = np.argwhere(X.expected(0)[1] == 0.0)[0]
    return int(q), int(s)


def pairs_ref(flags, rows, cols):
    """(I int32[P], D float64[P]): the oracle's cells (rows[p], cols[p])."""
    I, D = X.expected(flags)
    rows, cols = np.asarray(rows, np.int64), np.asarray(cols, np.int64)
    return np.ascontiguousarray(I[rows, cols], np.int32), np.ascontiguousarray(D[rows, cols], np.float64)


@functools.lru_cache(maxsize=None)
def lists():
    """name -> (rows into the queries, cols into the subjects), read-only int64 arrays."""
    rng = np.random.default_rng(20261021)
    out = {}
    # every query row at most once, shuffled
    out["singletons"] = (rng.permutation(NQ), rng.integers(0, NS, NQ))
    # one non-empty query against every subject among pairs of other rows
    r = np.concatenate([np.full(NS, LONG_ROW), rng.integers(LONG_ROW + 1, NQ, 60)])
    c = np.concatenate([np.arange(NS), rng.integers(0, NS, 60)])
    p = rng.permutation(len(r))
    out["long_group"] = (r[p], c[p])
    # rows with exactly 1, 63, 64, 65, 128 and 129 listed columns
    r, c = [], []
    for row, k in EDGE_ROWS.items():
        r += [row] * k
        c += rng.choice(NS, k, replace=False).tolist()
    p = rng.permutation(len(r))
    out["unit_edges"] = (np.array(r)[p], np.array(c)[p])
    # 2,000 pairs with replacement; planted: a repeated pair, the empty query x the subject without a
    # 21-mer, the empty query x a non-empty subject, a duplicate query x its subject
    r, c = rng.integers(0, NQ, 2000), rng.integers(0, NS, 2000)
    dq, ds = duplicate_pair()
    r[:5] = (REPEATED[0], REPEATED[0], EMPTY_Q, EMPTY_Q, dq)
    c[:5] = (REPEATED[1], REPEATED[1], KMERLESS_S, 0, ds)
    p = rng.permutation(2000)
    out["mixed"] = (r[p], c[p])
    res = {}
    for k, (a, b) in out.items():
        a, b = np.asarray(a, np.int64).copy(), np.asarray(b, np.int64).copy()
        a.setflags(write=False)
        b.setflags(write=False)
        res[k] = (a, b)
    return res


# ---- foreign cut -----------------------------------------------------------
FC_NS, FC_NQ = 6, 4
FC_WINDOW = (1 << 63) - (1 << 39), 1 << 40       # q0's window: first code, width
FC_PLANTED = (1, 4)                              # the subjects that hold 500 of q0's codes each
ALL_ONES = np.uint64(0xFFFFFFFFFFFFFFFF)


def _csr(sets):
    off = np.zeros(len(sets) + 1, np.int64)
    off[1:] = np.cumsum([len(s) for s in sets])
    codes = np.concatenate(sets).astype(np.uint64) if off[-1] else np.zeros(0, np.uint64)
    off.setflags(write=False)
    codes.setflags(write=False)
    return off, codes


@functools.lru_cache(maxsize=None)
def foreign_cut():
    """((subject offsets, codes), (query offsets, codes)): sorted distinct uint64 codes per set."""
    rng = np.random.default_rng(4096)
    subj = [np.unique(rng.integers(0, 1 << 64, 6000, dtype=np.uint64)) for _ in range(FC_NS)]
    inner = np.sort(np.concatenate(subj))
    lo, hi = int(inner[inner > 0].min()), int(inner[inner < ALL_ONES].max())
    q0 = np.uint64(FC_WINDOW[0]) + rng.choice(FC_WINDOW[1], 20000, replace=False).astype(np.uint64)
    q0 = np.sort(q0)
    for j in FC_PLANTED:
        subj[j] = np.unique(np.concatenate([subj[j], rng.choice(q0, 500, replace=False)]))
    # below every subject code but code 0, which subject 0 shares
    q1 = np.sort(np.concatenate([[0], 1 + rng.choice(lo - 1, 2999, replace=False)]).astype(np.uint64))
    # above every subject code but the all-ones code, which subject 0 shares
    top = ALL_ONES - np.uint64(1) - rng.choice((1 << 64) - 2 - hi, 2999, replace=False).astype(np.uint64)
    q2 = np.sort(np.concatenate([top, np.array([ALL_ONES], np.uint64)]))
    subj[0] = np.unique(np.concatenate([subj[0], np.array([0, ALL_ONES], np.uint64)]))
    return _csr(subj), _csr([q0, q1, q2, np.zeros(0, np.uint64)])


def _set(csr, i):
    off, codes = csr
    return codes[off[i]:off[i + 1]]


@functools.lru_cache(maxsize=None)
def foreign_cut_expected(flags=0):
    """(I[FC_NQ, FC_NS] int32, D float64): np.intersect1d and oracle.distance."""
    import oracle
    S, Q = foreign_cut()
    I = np.zeros((FC_NQ, FC_NS), np.int32)
    D = np.zeros((FC_NQ, FC_NS), np.float64)
    for i in range(FC_NQ):
        a = _set(Q, i)
        for j in range(FC_NS):
            b = _set(S, j)
            I[i, j] = len(np.intersect1d(a, b, assume_unique=True))
            D[i, j] = oracle.distance(int(I[i, j]), len(a), len(b), flags)
    I.setflags(write=False)
    D.setflags(write=False)
    return I, D


def check_fixture():
    """The conditions the GPU tests rely on, from the oracle's side only."""
    X.check_fixture()
    qn, sn = X.sizes()
    assert qn[EMPTY_Q] == 0 and sn[KMERLESS_S] == 0 and qn[LONG_ROW] > 0 and sn[0] > 0
    assert int(sn.max()) > 2 * 2048                       # the subjects' own index has nseg = 3
    L = lists()
    assert sorted(L) == ["long_group", "mixed", "singletons", "unit_edges"]
    for rows, cols in L.values():
        assert len(rows) == len(cols) and rows.min() >= 0 and rows.max() < NQ and cols.min() >= 0 and cols.max() < NS
    rows, cols = L["singletons"]
    assert len(rows) == NQ and len(np.unique(rows)) == NQ
    rows, cols = L["long_group"]
    mine = cols[rows == LONG_ROW]                         # in list order: the stable sort keeps it
    assert sorted(mine.tolist()) == list(range(NS)) and len(rows) == NS + 60 and len(np.unique(rows)) > 20
    # the budget is its minimum on a device of 64 CUs or more (8 units a CU) ...
    assert float((qn[rows] + sn[cols]).sum()) / (64 * 8) < UNIT_CODES_MIN
    # ... and every full chunk of the long row holds more than two budgets of codes: the cut makes > 1 unit of it
    for k in range(0, NS - UNIT + 1, UNIT):
        assert int(qn[LONG_ROW] + sn[mine[k:k + UNIT]].sum()) > 2 * UNIT_CODES_MIN
    rows, cols = L["unit_edges"]
    u, counts = np.unique(rows, return_counts=True)
    assert dict(zip(u.tolist(), counts.tolist())) == EDGE_ROWS
    assert sorted(counts.tolist()) == [1, 63, 64, 65, 128, 129]
    rows, cols = L["mixed"]
    pairs = list(zip(rows.tolist(), cols.tolist()))
    assert len(pairs) == 2000 and len(set(pairs)) < 2000 and pairs.count(REPEATED) >= 2
    dq, ds = duplicate_pair()
    for p in ((EMPTY_Q, KMERLESS_S), (EMPTY_Q, 0), (dq, ds)):
        assert p in pairs
    I, D = X.expected(0)
    assert D[dq, ds] == 0.0 and I[dq, ds] == qn[dq] == sn[ds] > 0
    assert np.isnan(X.expected(EMPTY_NAN)[1][EMPTY_Q, KMERLESS_S]) and D[EMPTY_Q, 0] == 1.0
    # foreign cut
    S, Q = foreign_cut()
    ssz, qsz = np.diff(S[0]), np.diff(Q[0])
    assert qsz.tolist() == [20000, 3000, 3000, 0]
    assert ssz.tolist() == [6002, 6500, 6000, 6000, 6500, 6000]
    for csr, n in ((S, FC_NS), (Q, FC_NQ)):
        for i in range(n):
            s = _set(csr, i)
            assert np.all(s[1:] > s[:-1])                 # sorted, distinct
    nseg_max = -(-int(ssz.max()) // 2048)
    assert nseg_max <= 4
    q0, q1, q2 = _set(Q, 0), _set(Q, 1), _set(Q, 2)
    assert int(q0[-1] - q0[0]) < FC_WINDOW[1] and int(q0[0]) >= FC_WINDOW[0]
    assert len(q0) > nseg_max * STAGE                     # whatever splitters fall inside, one segment > STAGE
    allc = np.concatenate([_set(S, j) for j in range(FC_NS)])
    assert q1[0] == 0 and np.all(q1[1:] < allc[allc > 0].min())
    assert q2[-1] == ALL_ONES and np.all(q2[:-1] > allc[allc < ALL_ONES].max())
    I, D = foreign_cut_expected(0)
    assert I[0].tolist() == [0, 500, 0, 0, 500, 0]
    assert I[1].tolist() == [1, 0, 0, 0, 0, 0] and I[2].tolist() == [1, 0, 0, 0, 0, 0] and not I[3].any()
    assert np.all(D[3] == 1.0) and D[0, 1] < 1.0
