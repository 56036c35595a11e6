"""In-group / out-group distance summary on the device (gdist_group_stats): the
distCheck report of DistanceCheckProcessor.java:149-223 over a device-resident
collection. Every integer field (counts, the exact sums of m = d * 2^53 and
m * m, bad pairs) and the bits of min / max are compared with `==` against
group_ref on the oracle's distance matrix; mean must lie within 1 ulp and sdev
within 2 ulp of the exact Fractions (the bounds of the host arithmetic: one
division of two values rounded to 64 bits, one rounding to fp64, and a square
root). Outputs are pre-filled with garbage, so a field the call leaves
unwritten fails. Each property of the fixture a test relies on is asserted
on the oracle's matrix first."""
import ctypes as C
import functools
import io
from fractions import Fraction

import numpy as np
import pytest

import closest_ref as R
import group_ref as G
import oracle

pytestmark = pytest.mark.gpu

N = 195
EMPTY_NAN, SKETCH_JACCARD, UPPER_TRIANGLE, OUT_DEVICE = 0x400, 0x800, 0x100, 0x200
TYPES = ("block", "one", "solo", "holes")


def make_labels(n):
    i = np.arange(n)
    return np.stack([i // 15, np.zeros(n, dtype=np.int64), i, np.where(i % 7 == 0, -1, i % 3)]).astype(np.int32)


LABELS = make_labels(N)


def raw_stats(sets, labels, rows=None, cols=None, upper=True, method=0, flags=0):
    """gdist_group_stats into garbage-filled outputs: (rc, sides [2 T], bad [T])."""
    from gdist import _lib as L
    labels = np.ascontiguousarray(np.atleast_2d(labels), dtype=np.int32)
    T, ns = labels.shape[0], len(sets)
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    sides, bad = (L.GroupSide * (2 * T))(), (C.c_int64 * T)(*([-9] * T))
    C.memset(sides, 0xA5, C.sizeof(sides))
    fl = flags | (UPPER_TRIANGLE if upper else 0)
    rc = L.lib.gdist_group_stats(sets.ctx.h, sets.h, r0, r1, c0, c1, method, fl, T, L.ptr(labels, C.c_int32),
                                 C.addressof(sides), bad)
    return rc, sides, bad


def raw_bytes(*a, **kw):
    rc, sides, bad = raw_stats(*a, **kw)
    assert rc == 0
    return bytes(sides) + bytes(bad)


@functools.lru_cache(maxsize=None)
def recipe_ref(rows=None, cols=None, upper=True, flags=0):
    """group_ref on the oracle's matrix of the recipe, once per region."""
    D = R.recipe(flags)[3]
    r0, r1 = rows or (0, N)
    c0, c1 = cols or (0, N)
    return G.group_ref(D[r0:r1, c0:c1], LABELS, r0, c0, upper)


def check(sets, D, labels, rows=None, cols=None, upper=True, method=0, flags=0, ref=None):
    ns = D.shape[0]
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    rc, sides, bad = raw_stats(sets, labels, rows, cols, upper, method, flags)
    assert rc == 0
    if ref is None:
        ref = G.group_ref(D[r0:r1, c0:c1], labels, r0, c0, upper)
    G.check_stats(sides, bad, ref, f"rows {rows} cols {cols} upper {upper} method {method}")
    return bytes(sides) + bytes(bad)


@pytest.fixture(scope="module")
def kset(ctx):
    import gdist
    seqs, _, _, D = R.recipe()
    assert D.shape == (N, N)
    s = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


def test_fixture_properties():
    """What the tests below rely on, on the oracle's matrix."""
    up, full = recipe_ref(upper=True), recipe_ref(upper=False)
    side = lambda ref, t, k: ref[TYPES.index(t)]["sides"][k]
    assert (side(up, "block", 0)["n"], side(up, "block", 0)["ones"]) == (1053, 312)
    assert (side(up, "block", 1)["n"], side(up, "block", 1)["ones"]) == (10575, 6975)
    assert side(up, "block", 1)["sum"] >> 66 == 1                     # its sum needs 67 bits: a second limb
    assert side(up, "one", 1)["n"] == 0 and side(up, "solo", 0)["n"] == 0
    assert up[TYPES.index("holes")]["bad"] == 5054
    s = side(full, "solo", 0)
    assert (s["n"], s["ones"], s["min"], s["max"]) == (193, 2, 0.0, 0.0)
    assert (side(full, "one", 0)["n"], side(full, "one", 0)["ones"]) == (23449, 14576)
    assert full[TYPES.index("holes")]["bad"] == 10136
    assert all(r["sides"][k]["nans"] == 0 for r in up + full for k in range(2))


@pytest.mark.parametrize("upper", [True, False], ids=["upper", "full"])
@pytest.mark.parametrize("method", [1, 2, 0], ids=["sorted", "bitset", "auto"])
def test_methods_and_regions(kset, method, upper):
    D = R.recipe()[3]
    got = check(kset, D, LABELS, upper=upper, method=method, ref=recipe_ref(upper=upper))
    assert raw_bytes(kset, LABELS, upper=upper, method=method) == got          # a second call: identical bytes
    assert raw_bytes(kset, LABELS, upper=upper, method=1) == got               # and whatever the method


@pytest.mark.parametrize("rows_,cols_", [(7, 33), (64, 100), (128, 193), (1, 64)])
def test_block_sizes(kset, opts, rows_, cols_):
    """Several row blocks and column chunks, ragged last ones, chunks left of,
    on and right of the diagonal: the struct array does not depend on them."""
    assert N % cols_ != 0 and N > cols_
    want = {u: raw_bytes(kset, LABELS, upper=u) for u in (True, False)}
    opts(closest_rows=rows_, closest_cols=cols_)
    for u in (True, False):
        for method in ((1, 2) if rows_ > 1 else (0,)):     # one row a block: 780 steps a call
            assert raw_bytes(kset, LABELS, upper=u, method=method) == want[u]


def test_rectangles(kset):
    D = R.recipe()[3]
    for method in (1, 2):
        for upper in (True, False):
            check(kset, D, LABELS, rows=(3, 77), cols=(50, 160), upper=upper, method=method,
                  ref=recipe_ref((3, 77), (50, 160), upper))
        check(kset, D, LABELS, rows=(150, 195), cols=(0, 150), upper=False, method=method,
              ref=recipe_ref((150, 195), (0, 150), False))
    # wholly left of the diagonal: no pair, every side in its n == 0 form, bad 0
    ref = recipe_ref((100, 195), (0, 100), True)
    assert all(r["bad"] == 0 and r["sides"][k][f] == 0 for r in ref for k in range(2) for f in ("n", "ones", "nans"))
    got = check(kset, D, LABELS, rows=(100, 195), cols=(0, 100), upper=True, ref=ref)
    import gdist
    assert got == gdist.GroupStats.empty(4).tobytes()
    # empty ranges answer the same
    assert raw_bytes(kset, LABELS, rows=(5, 5)) == got and raw_bytes(kset, LABELS, rows=(5, 9), cols=(20, 20)) == got


def test_empty_nan(kset):
    """Two empty sets: NaN from each other and themselves with GDIST_EMPTY_NAN,
    counted apart from the statistics."""
    D = R.recipe(EMPTY_NAN)[3]
    assert int(np.isnan(D).sum()) == 4
    for method in (1, 2):
        for upper, nans in ((False, 4), (True, 1)):
            ref = recipe_ref(upper=upper, flags=EMPTY_NAN)
            assert ref[TYPES.index("one")]["sides"][0]["nans"] == nans
            rc, sides, bad = raw_stats(kset, LABELS, upper=upper, method=method, flags=EMPTY_NAN)
            assert rc == 0 and sides[2 * TYPES.index("one")].nans == nans
            G.check_stats(sides, bad, ref)
    assert recipe_ref(upper=False)[1]["sides"][0]["ones"] == recipe_ref(upper=False, flags=EMPTY_NAN)[1]["sides"][0]["ones"] + 4


def test_protein(ctx):
    import gdist
    from gdist import synth
    prots = [bytes(r) for r in synth.genomes(60, 400, 0.1, 43, protein=True)]
    off, codes = oracle.pack(prots, 8, 1, 0)
    _, D = oracle.matrix(off, codes, 0, 60, 0, 60)
    lab = make_labels(60)
    ref = G.group_ref(D, lab, upper=True)
    assert ref[0]["sides"][0]["n"] > 1 and ref[0]["sides"][1]["n"] > 1
    s = gdist.KmerSets.from_sequences(prots, 8, gdist.KmerType.PROT, 0, ctx)
    for method in (1, 2):
        check(s, D, lab, method=method, ref=ref)
        check(s, D, lab, upper=False, method=method)
    s.free()


@pytest.fixture(scope="module")
def sketch_case(ctx):
    """The first 120 sequences of the recipe and one of 100 bp (a dwarf at
    width 200); per width the collection and the oracle's signatures."""
    import gdist
    from gdist import synth
    seqs = R.recipe_sequences()[:120] + [bytes(synth.genomes(1, 100, 0.0, 7)[0])]
    off, codes = oracle.pack(seqs, 21, 0, 0)
    ks = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    out = {}
    for width in (64, 200):
        sigs = [oracle.sketch(codes[off[i]:off[i + 1]], 21, 0, width) for i in range(len(seqs))]
        out[width] = (ks.sketches(width), sigs)
    assert len(out[200][1][120]) < 200 and len(out[64][1][120]) == 64
    yield out
    for sk, _ in out.values():
        sk.free()
    ks.free()


@pytest.mark.parametrize("flags", [0, SKETCH_JACCARD], ids=["mash", "jaccard"])
@pytest.mark.parametrize("width", [64, 200])
def test_sketches(sketch_case, opts, width, flags):
    sk, sigs = sketch_case[width]
    m = len(sigs)
    D = np.array([[oracle.sketch_distance(sigs[i], sigs[j], width, flags)[0] for j in range(m)] for i in range(m)])
    lab = make_labels(m)
    ref = G.group_ref(D, lab, upper=True)
    assert ref[0]["sides"][0]["n"] > 1 and ref[0]["sides"][1]["n"] > 1
    got = check(sk, D, lab, flags=flags, ref=ref)
    assert raw_bytes(sk, lab, flags=flags, method=77) == got                   # sketches ignore the method
    full = check(sk, D, lab, upper=False, flags=flags)
    check(sk, D, lab, rows=(100, 121), cols=(0, 100), upper=False, flags=flags)
    opts(closest_rows=50, closest_cols=37)
    assert raw_bytes(sk, lab, flags=flags) == got and raw_bytes(sk, lab, upper=False, flags=flags) == full
    st = sk.group_stats(lab, flags=flags)
    assert st.tobytes() == got


def test_type_counts(kset):
    """T = 1 and T = 8: each grouping's answer does not depend on its neighbours."""
    D = R.recipe()[3]
    ref = recipe_ref(upper=True)
    for t in range(4):
        check(kset, D, LABELS[t], ref=[ref[t]])
    lab8 = np.concatenate([LABELS[::-1], LABELS])
    check(kset, D, lab8, ref=ref[::-1] + ref)


def test_merge_rows(kset):
    """Two row shards merged on the host equal the single call, byte for byte."""
    for upper in (True, False):
        whole = kset.group_stats(LABELS, upper=upper)
        a = kset.group_stats(LABELS, rows=(0, 100), upper=upper)
        b = kset.group_stats(LABELS, rows=(100, N), upper=upper)
        assert whole.tobytes() == raw_bytes(kset, LABELS, upper=upper)
        assert a.merge(b).tobytes() == whole.tobytes() and b.merge(a).tobytes() == whole.tobytes()
        assert a.tobytes() != whole.tobytes()
    assert whole.n.shape == (4, 2) and whole.bad.tolist() == [r["bad"] for r in recipe_ref(upper=False)]
    assert whole.sum[0][1] == recipe_ref(upper=False)[0]["sides"][1]["sum"]


def test_third_limb(ctx):
    """4096 sets {0, i + 1}: every pair shares one kmer of three, d = fl(1 -
    fl(1 / 3)) off the diagonal and 0.0 on it; over the full region the sum of
    squares passes 2^128. Expected values in closed form."""
    import gdist
    n = 4096
    off = np.arange(n + 1, dtype=np.int64) * 2
    codes = np.stack([np.zeros(n, dtype=np.uint64), np.arange(1, n + 1, dtype=np.uint64)], axis=1).ravel()
    d = 1.0 - 1.0 / 3.0
    (m,) = G.exact_m([d])
    lab = np.stack([np.zeros(n, dtype=np.int32), (np.arange(n) % 2).astype(np.int32)])

    def side(pairs, diag):
        """`pairs` off-diagonal pairs at d and `diag` diagonal ones at 0.0."""
        cnt, s, q = pairs + diag, pairs * m, pairs * m * m
        return {"n": cnt, "ones": 0, "nans": 0, "sum": s, "sumsq": q, "min": 0.0 if diag else d, "max": d,
                "mean": Fraction(s, cnt * G.TWO53),
                "var": Fraction(cnt * q - s * s, cnt * (cnt - 1) * G.TWO53 ** 2)}
    same = 2 * (n // 2) * (n // 2 - 1)                 # ordered off-diagonal pairs of equal parity
    ref = [{"bad": 0, "sides": [side(n * (n - 1), n), G.side_ref([])]},
           {"bad": 0, "sides": [side(same, n), side(n * n - n - same, 0)]}]
    assert ref[0]["sides"][0]["sumsq"] >> 128 != 0      # sumsq[2] != 0
    s = gdist.KmerSets.from_codes(off, codes, 21, gdist.KmerType.DNA, ctx)
    rc, sides, bad = raw_stats(s, lab, upper=False)
    assert rc == 0 and sides[0].sumsq[2] != 0
    G.check_stats(sides, bad, ref)
    s.free()


def test_errors_leave_the_outputs_untouched(kset, ctx):
    import gdist
    from gdist import _lib as L
    garbage = bytes([0xA5]) * (8 * 96) + np.full(4, -9, dtype=np.int64).tobytes()

    def einval(*a, **kw):
        rc, sides, bad = raw_stats(*a, **kw)
        assert rc == L.EINVAL and L.lib.gdist_last_error()
        assert bytes(sides) + bytes(bad) == garbage

    einval(kset, LABELS, rows=(0, N + 1))
    einval(kset, LABELS, rows=(-1, 5))
    einval(kset, LABELS, rows=(9, 5))
    einval(kset, LABELS, cols=(0, N + 1))
    einval(kset, LABELS, cols=(7, 3))
    einval(kset, LABELS, flags=OUT_DEVICE)
    einval(kset, LABELS, method=3)
    sides, bad = (L.GroupSide * 18)(), (C.c_int64 * 9)()
    lab9 = np.zeros((9, N), dtype=np.int32)
    args = (ctx.h, kset.h, 0, N, 0, N, 0, 0)
    for T in (0, 9, -1):
        assert L.lib.gdist_group_stats(*args, T, L.ptr(lab9, C.c_int32), C.addressof(sides), bad) == L.EINVAL
    assert L.lib.gdist_group_stats(*args, 1, None, C.addressof(sides), bad) == L.EINVAL
    assert L.lib.gdist_group_stats(*args, 1, L.ptr(lab9, C.c_int32), None, bad) == L.EINVAL
    assert L.lib.gdist_group_stats(*args, 1, L.ptr(lab9, C.c_int32), C.addressof(sides), None) == L.EINVAL
    assert L.lib.gdist_group_stats(ctx.h, None, 0, 2, 0, 2, 0, 0, 1, L.ptr(lab9, C.c_int32), C.addressof(sides),
                                   bad) == L.EINVAL
    assert not any(bytes(sides)) and not any(bad)
    with pytest.raises(ValueError):
        kset.group_stats(LABELS[:, :10])
    with pytest.raises(ValueError):
        kset.group_stats(lab9)
    # a bitsets-only collection: SORTED is refused, BITSET and AUTO answer
    b = gdist.KmerSets.from_sequences(R.recipe_sequences(), 21, gdist.KmerType.DNA, 0, ctx)
    b.build_bitsets()
    b.release_codes()
    einval(b, LABELS, method=1)
    want = raw_bytes(kset, LABELS)
    assert raw_bytes(b, LABELS, method=2) == want and raw_bytes(b, LABELS, method=0) == want
    b.free()


def test_timing_option(kset, ctx, opts):
    assert raw_bytes(kset, LABELS) and ctx.group_stats_timing() == (-1.0, -1.0)
    opts(time_kernels=1)
    want = raw_bytes(kset, LABELS)
    matrix_ms, reduce_ms = ctx.group_stats_timing()
    assert matrix_ms > 0 and reduce_ms > 0
    opts(time_kernels=0)
    assert raw_bytes(kset, LABELS) == want and ctx.group_stats_timing() == (-1.0, -1.0)


def test_distance_check_tsv(kset):
    """processors.distance_check: the distCheck table equals the text built
    from group_ref (min, max and ones exactly; low, mean and high through the
    call's own mean / sdev, each checked against the Fractions above)."""
    from gdist import java_double, processors
    ids = [f"83333.{i}" for i in range(N)]
    groupings = {name: {ids[i]: f"grp{LABELS[t, i]}" for i in range(N) if LABELS[t, i] >= 0}
                 for t, name in enumerate(TYPES)}
    names, lab = processors.group_labels(ids, groupings)
    assert names == list(TYPES) and np.array_equal(lab[:3], LABELS[:3])
    assert np.array_equal(lab[3] < 0, LABELS[3] < 0)
    for upper in (True, False):
        ref = recipe_ref(upper=upper)
        st = kset.group_stats(LABELS, upper=upper)
        G.check_stats(st.sides, st.bad_raw, ref)
        out = io.StringIO()
        assert processors.distance_check(kset, ids, groupings, out, "recipe.tbl", upper=upper) == \
            sum(r["bad"] for r in ref)
        lines = ["dist_file\tgroup_type\tin_out\tmin\tlow\tmean\thigh\tmax\tones"]
        for t, r in enumerate(ref):
            for k, s in enumerate(r["sides"]):
                if s["n"] == 0:
                    vals = [1.0] * 5
                else:
                    vals = [s["min"], st.mean[t, k] - st.sdev[t, k], st.mean[t, k], st.mean[t, k] + st.sdev[t, k],
                            s["max"]]
                lines.append("\t".join(["recipe.tbl", TYPES[t], ("in", "out")[k]] +
                                       [java_double(float(v)) for v in vals] + [str(s["ones"])]))
        assert out.getvalue() == "\n".join(lines) + "\n"
        if upper:
            assert "recipe.tbl\tsolo\tin\t1.0\t1.0\t1.0\t1.0\t1.0\t0\n" in out.getvalue()    # no pair in the side
        else:
            assert "recipe.tbl\tsolo\tin\t0.0\t0.0\t0.0\t0.0\t0.0\t2\n" in out.getvalue()    # the diagonal
    out2 = io.StringIO()
    processors.distance_check(kset, ids, groupings, out2, "recipe.tbl", header=False, upper=False)
    assert out2.getvalue() == "".join(out.getvalue().splitlines(True)[1:])
