"""gdist_pairs and gdist_sketch_pairs share one plan (csrc/pair_list.hip) and
the context's pairs_info fields: alternated on one context, each call answers
its reference bit for bit and reports its own numbers, whatever ran before."""
import numpy as np
import pytest

import closest_ref as CR
import pairs_ref as KR
import sketch_pairs_ref as SR

pytestmark = pytest.mark.gpu

SORTED, BITSET = 1, 2
WIDTH = 65
UNIT_CODES_MIN = 1 << 14     # the least code budget of a sorted unit (csrc/pair_list.hpp)


def test_alternated_calls_share_the_context(ctx):
    import gdist
    seqs, off, _, _ = CR.recipe()
    subj, qry = SR.sides(WIDTH)
    kset = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    S, Q = (gdist.SketchSets.from_signatures(x, WIDTH, ctx) for x in (subj, qry))
    try:
        kr, kc = KR.recipe_lists()["unit_edges"]
        sr, sc = SR.runs_and_singles()
        kI, kD = KR.pairs_ref(*KR.recipe_matrices(), kr, kc)
        exp = SR.expected(WIDTH, 0)
        sI, sD = exp[0][sr, sc], exp[1][sr, sc]
        counts = np.unique(kr, return_counts=True)[1]
        chunks = int(((counts + 63) // 64).sum())
        assert chunks > len(counts) and SR.unit_count(sr) > len(np.unique(sr))   # both lists hold rows past a unit
        # gdist.h: a sorted unit is a row, at most 64 of its pairs and a range of the segment index; a
        # chunk is cut once per budget of its codes, and no budget is below UNIT_CODES_MIN
        sizes = np.diff(off)
        cut_most = chunks + int((sizes[kr] + sizes[kc]).sum()) // UNIT_CODES_MIN

        I, D = kset.pairs(kr, kc, method=SORTED)
        assert np.array_equal(I, kI) and np.array_equal(SR.bits(D), SR.bits(kD))
        ms, groups, units = kset.pairs_info()
        assert ms == -1.0 and groups == len(counts) and chunks <= units <= cut_most

        common, D = Q.pairs(sr, sc, other=S)
        assert np.array_equal(common, sI) and np.array_equal(SR.bits(D), SR.bits(sD))
        assert Q.pairs_info() == (-1.0, len(np.unique(sr)), SR.unit_count(sr))

        I, D = kset.pairs(kr, kc, method=BITSET)
        assert np.array_equal(I, kI) and np.array_equal(SR.bits(D), SR.bits(kD))
        assert kset.pairs_info() == (-1.0, len(counts), len(kr))            # a unit a pair

        common, D = Q.pairs(sr, sc, other=S, want_common=False)
        assert common is None and np.array_equal(SR.bits(D), SR.bits(sD))
        assert Q.pairs_info() == (-1.0, len(np.unique(sr)), SR.unit_count(sr))
    finally:
        for h in (kset, S, Q):
            h.free()
