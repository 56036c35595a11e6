"""Shared fixture of the cross-collection tests (gdist_cross_matrix /
gdist_cross_closest): numpy plus the oracle, no call into the library. Used by
test_cross_host.py (CPU) and test_gpu_cross.py.

The 195-sequence recipe of closest_ref.py (DNA, k = 21) is split into a
resident collection of 143 subjects (blocks of 64 + 64 + 15 columns) and 52
queries; the expected matrices are the oracle's I and D sliced to queries x
subjects. The queries hold three exact duplicates of subjects 5 and 77,
unrelated genomes and the empty sequence; the last subject has no 21-mer.
"""
import functools

import numpy as np

import closest_ref as R

SUBJECTS = list(range(0, 120)) + list(range(153, 175)) + [194]
QUERIES = list(range(120, 153)) + list(range(175, 194))
NS, NQ = len(SUBJECTS), len(QUERIES)
EMPTY_NAN = 0x400


def sequences():
    """(subject sequences, query sequences)."""
    seqs = R.recipe_sequences()
    return [seqs[i] for i in SUBJECTS], [seqs[i] for i in QUERIES]


@functools.lru_cache(maxsize=None)
def expected(flags=0):
    """(I[NQ, NS] int32, D[NQ, NS] float64) of the oracle with `flags`. Read-only."""
    import oracle
    _, off, codes, _ = R.recipe()
    n = len(off) - 1
    I, D = oracle.matrix(off, codes, 0, n, 0, n, flags=flags)
    I = np.ascontiguousarray(I[np.ix_(QUERIES, SUBJECTS)])
    D = np.ascontiguousarray(D[np.ix_(QUERIES, SUBJECTS)])
    I.setflags(write=False)
    D.setflags(write=False)
    return I, D


@functools.lru_cache(maxsize=None)
def packed():
    """(offsets, codes) of the oracle's pack of subjects + queries, in that
    order: the collection gdist_sets_concat(subjects, queries) holds."""
    import oracle
    subj, qry = sequences()
    off, codes = oracle.pack(subj + qry, 21, 0, 0)
    off.setflags(write=False)
    codes.setflags(write=False)
    return off, codes


def sizes():
    """(query set sizes, subject set sizes)."""
    n = np.diff(packed()[0])
    return n[NS:], n[:NS]


def check_fixture():
    """The conditions the cross tests rely on; a recipe that stopped
    exercising them fails here instead of passing quietly."""
    import oracle
    assert (NS, NQ) == (143, 52) and sorted(SUBJECTS + QUERIES) == list(range(195))
    I, D = expected(0)
    off, codes = packed()
    cI, cD = oracle.matrix(off, codes, NS, NS + NQ, 0, NS, flags=0)
    assert np.array_equal(I, cI) and np.array_equal(D.view(np.uint64), cD.view(np.uint64))
    assert int((D < 1.0).sum()) == 3960 and D.size == 7436
    assert int((D == 0.0).sum()) == 3
    In, Dn = expected(EMPTY_NAN)
    assert np.array_equal(In, I)
    nan = np.argwhere(np.isnan(Dn))
    assert nan.tolist() == [[NQ - 1, NS - 1]]          # the empty query x the subject without a 21-mer
    qn, sn = sizes()
    assert qn[NQ - 1] == 0 and sn[NS - 1] == 0
    assert int(max(qn.max(), sn.max())) == 5960        # nseg = ceil(5960 / 2048) = 3
    assert int(I.max()) == 5960
    _, _, c = R.closest_ref(D, 10, 0.9, keep_self=True)
    assert (int((c == 10).sum()), int(((c > 0) & (c < 10)).sum()), int((c == 0).sum())) == (30, 2, 20)
    _, _, c = R.closest_ref(D, 10, 1.0, keep_self=True)
    assert np.all(c == 10)
    s = np.sort(D, axis=1)
    assert int((s[:, 9] == s[:, 10]).sum()) == 20      # the (d, column) order decides the 10th neighbour
    _, _, c = R.closest_ref(D, 10, 0.0, keep_self=True)
    assert int((c == 1).sum()) == 3 and int((c == 0).sum()) == NQ - 3
