"""CPU: what test_gpu_lifecycle.py relies on, checked without a device. The
pool of lifecycle_ref meets, on the oracle's matrix alone, the conditions its
tests need (literals read from that matrix); the walks of lifecycle_ref.SEEDS
deal every legal (mutation, consumer) pair among them and each holds an
append that must reallocate the code buffer and one that fits in place;
concat is bound on both handle classes and refuses a null handle."""
import ctypes as C
import os
import re

import numpy as np

import lifecycle_ref as LR

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_fixture_properties():
    """Conditions, not measurements: the pool was chosen so that the oracle alone meets them."""
    p = LR.pool("dna")
    n, R = p.n, LR.N_REL
    assert n == 200
    offd = ~np.eye(n, dtype=bool)
    rel = p.I[:R, :R][~np.eye(R, dtype=bool)]
    assert int((rel > 0).sum()) == 22350 and 2 * int((rel > 0).sum()) >= rel.size     # related sets share kmers
    assert int(((p.D == 0.0) & offd).sum()) == 10                                     # exact duplicates
    assert int(((p.D == 1.0) & offd).sum()) == 16082                                  # disjoint pairs
    assert np.flatnonzero(p.sizes == 0).tolist() == [193, 194]                        # two empty sets
    row = p.D[0, 1:R]
    assert int((row < 1.0).sum()) == 149 and len(np.unique(row)) == 133               # natural ties in row 0
    assert (int(p.sizes.max()), float(np.median(p.sizes))) == (59972, 5972.0)
    assert p.sizes.max() >= 8 * np.median(p.sizes)
    # the model of a collection is the pool's own rows and codes
    idx = [7, 150, 193, 7, 199]
    off, codes = p.csr(idx)
    assert off.tolist() == [0] + np.cumsum(p.sizes[idx]).tolist()
    assert np.array_equal(codes[off[3]:off[4]], p.sets[7]) and np.array_equal(codes[off[4]:], p.sets[199])
    I, D = p.matrices(idx)
    assert D[0, 3] == 0.0 and I[0, 3] == p.sizes[7] and D[2, 2] == 1.0


def test_walks_cover_every_pair():
    """Over SEEDS every legal (mutation kind, consumer kind) pair occurs; a
    release is followed only by consumers that need no codes, then by a pack."""
    seen = set()
    for seed in LR.SEEDS:
        ops = LR.walk(seed, LR.STEPS)
        assert ops[0]["op"] == "pack" and ops == LR.walk(seed, LR.STEPS)              # deterministic
        body = [o for o in ops if o["op"] != "pack"]
        assert len(body) == 2 * LR.STEPS
        for m, c in zip(body[0::2], body[1::2]):
            assert m["op"] in LR.MUTATIONS and c["op"] in LR.CONSUMERS and m["idx"] == c["idx"]
            seen.add((m["op"], c["op"]))
        for i, o in enumerate(ops):
            if o["op"] == "release":
                assert ops[i + 1]["op"] not in LR.NEEDS_CODES
                assert i + 2 == len(ops) or ops[i + 2]["op"] == "pack"
            assert len(o["idx"]) <= 300
    assert seen == set(LR.legal_pairs()) and len(seen) == 6 * 11 - 2


def test_walks_append_in_place_and_by_reallocation():
    """gdist_sets_append grows the codes in place while the buffer has room and
    moves them to a buffer of twice the need otherwise. A batch of more codes
    than the collection holds cannot fit in place whatever the buffer's slack
    was; the single set appended right after it fits the doubled buffer."""
    p = LR.pool("dna")
    for seed in LR.SEEDS:
        ops = LR.walk(seed, LR.STEPS)
        app = [(i, o) for i, o in enumerate(ops) if o["op"] == "append"]
        assert any(o["realloc"] is True for _, o in app) and any(o["realloc"] is False for _, o in app), seed
        i0, first = app[0]
        i1, second = app[1]
        before = int(p.sizes[ops[i0 - 1]["idx"]].sum())
        add = int(p.sizes[first["batch"]].sum())
        assert first["realloc"] is True and add > before
        # the grown buffer holds 2 (before + add) codes; the next batch is one set
        assert second["realloc"] is False and len(second["batch"]) == 1
        assert before + add + int(p.sizes[second["batch"]].sum()) <= 2 * (before + add)
        assert i1 == i0 + 2


def test_expected_answers_follow_the_header():
    """any_le is <= t (a t equal to a distance hits); argmin is strict < 1.0
    with ties to the lowest position, a repeated column at its first place."""
    row = [0.5, 0.25, 1.0, 0.25, 0.75]
    assert LR.any_le_ref(row, 0.25) and not LR.any_le_ref(row, float(np.nextafter(0.25, 0)))
    assert not LR.any_le_ref([], 1.0) and not LR.any_le_ref(row, -1.0)
    assert LR.argmin_ref(row) == (1, 0.25)
    assert LR.argmin_ref([1.0, 1.0]) == (-1, 1.0) and LR.argmin_ref([]) == (-1, 1.0)
    D = np.array([[0.0, 0.2, 0.9, 1.0], [0.2, 0.0, 0.2, 1.0], [0.9, 0.2, 0.0, 0.5], [1.0, 1.0, 0.5, 0.0]])
    reps, rep_of, rep_d = LR.greedy_ref(D, 0.2)
    assert reps == [0, 2, 3] and rep_of.tolist() == [0, 0, 2, 3] and rep_d.tolist() == [0.0, 0.2, 0.0, 0.0]


def test_concat_is_bound_on_both_handle_classes():
    import gdist
    from gdist import kmers
    assert kmers.KmerSets.concat is kmers._Handle.concat and kmers.SketchSets.concat is kmers._Handle.concat
    assert "concat" not in vars(kmers.KmerSets) and gdist.SketchSets is kmers.SketchSets
    header = open(os.path.join(ROOT, "include", "gdist.h")).read()
    assert re.search(r"\bint\s+gdist_sets_concat\s*\(", re.sub(r"/\*.*?\*/", "", header, flags=re.S))


def test_concat_and_append_null_handles_are_einval():
    from gdist import _lib
    out = C.c_void_p(0x5A5A)
    _lib.lib.gdist_triangle_partition(-1, 4, 1, _lib.ptr(np.zeros(5, np.int64), C.c_int64))   # another message first
    assert _lib.lib.gdist_sets_concat(None, None, C.byref(out)) == _lib.EINVAL
    assert b"null sets handle" in _lib.lib.gdist_last_error()
    assert out.value == 0x5A5A                                                       # nothing was written
    first = C.c_int64(-9)
    off = np.zeros(2, np.int64)
    assert _lib.lib.gdist_sets_append(None, None, b"A", _lib.ptr(off, C.c_int64), 1, C.byref(first)) == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error() and first.value == -9
    assert _lib.lib.gdist_sets_release_codes(None) == _lib.EINVAL
    assert b"null sets handle" in _lib.lib.gdist_last_error()
