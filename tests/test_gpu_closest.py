"""Exact nearest neighbours on the device (gdist_closest): getClosest(kmers, n,
maxDist) of MashProcessor.java:150 / FindProcessor.java:110 over every column.
Every answer is compared with `==` (indices, fp64 bits of the distances,
counts and the unused slots) against a full sort of the oracle's distance
matrix (closest_ref), whatever the method, the block sizes and the region.
The outputs are pre-filled with garbage, so a slot the call leaves unwritten
fails. Each property of the fixture a test relies on is asserted on the
oracle's matrix first."""
import ctypes as C
import io

import numpy as np
import pytest

import closest_ref as R
import oracle

pytestmark = pytest.mark.gpu

N = 195
EMPTY_NAN, SKETCH_JACCARD, UPPER_TRIANGLE, OUT_DEVICE, KEEP_SELF = 0x400, 0x800, 0x100, 0x200, 0x1000


def raw_closest(sets, n, max_dist, rows=None, cols=None, method=0, flags=0):
    """gdist_closest into garbage-filled outputs: (rc, idx[nr, n], d[nr, n], count[nr])."""
    from gdist import _lib as L
    ns = len(sets)
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    nr = max(r1 - r0, 0)
    idx = np.full(max(nr * n, 1), 0x5A5A5A5A5A5A5A5A, dtype=np.int64)
    d = np.full(max(nr * n, 1), 7.5, dtype=np.float64)
    cnt = np.full(max(nr, 1), -9, dtype=np.int32)
    rc = L.lib.gdist_closest(sets.ctx.h, sets.h, r0, r1, c0, c1, method, flags, n, max_dist,
                             L.ptr(idx, C.c_int64), L.ptr(d, C.c_double), L.ptr(cnt, C.c_int32))
    return rc, idx[:nr * n].reshape(nr, n), d[:nr * n].reshape(nr, n), cnt[:nr]


def check(sets, D, n, max_dist, rows=None, cols=None, method=0, flags=0):
    """The call equals closest_ref on D (the oracle's matrix of the whole collection)."""
    ns = D.shape[0]
    r0, r1 = rows or (0, ns)
    c0, c1 = cols or (0, ns)
    rc, idx, d, cnt = raw_closest(sets, n, max_dist, rows, cols, method, flags)
    assert rc == 0
    eidx, ed, ecnt = R.closest_ref(D[r0:r1, c0:c1], n, max_dist, r0, c0, keep_self=bool(flags & KEEP_SELF))
    assert np.array_equal(cnt, ecnt)
    assert np.array_equal(idx, eidx)
    assert np.array_equal(d.view(np.uint64), ed.view(np.uint64))
    return idx, d, cnt


@pytest.fixture(scope="module")
def kset(ctx):
    import gdist
    seqs, _, _, D = R.recipe()
    assert D.shape == (N, N)
    s = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    yield s
    s.free()


def _candidates(D, max_dist):
    with np.errstate(invalid="ignore"):
        return ((D <= max_dist) & ~np.eye(len(D), dtype=bool)).sum(1)


def test_fixture_properties():
    """What the tests below rely on, on the oracle's matrix."""
    _, off, _, D = R.recipe()
    offd = ~np.eye(N, dtype=bool)
    assert int(((D == 0.0) & offd).sum()) == 8
    assert int(((D == 1.0) & offd).sum()) == 14574
    assert len(np.unique(D[0, 1:150])) == 129                     # natural ties in row 0
    c9 = _candidates(D, 0.9)
    assert int((c9 < 10).sum()) == 52 and int((c9 >= 70).sum()) == 71
    assert np.all(_candidates(D, 1.0) == N - 1)
    assert ((D == 1.0) & offd).sum(1).min() == 42                  # the tie group at 1.0 exceeds any n < 42
    assert np.diff(off)[-2:].tolist() == [0, 0]                    # two empty sets


SIZES = [(1, 0.9), (10, 0.5), (10, 0.9), (64, 0.97), (65, 1.0), (200, 1.0), (512, 1.0)]


@pytest.mark.parametrize("method", [1, 2], ids=["sorted", "bitset"])
@pytest.mark.parametrize("n,max_dist", SIZES)
def test_methods_and_sizes(kset, method, n, max_dist):
    """n below, at and above one wave (64), and above N; lists shorter than n,
    full lists and the large tie group at 1.0."""
    D = R.recipe()[3]
    c = _candidates(D, max_dist)
    if n in (10, 64):
        assert (c < n).any() and (c > n).any()
    if n >= 200:
        assert np.all(c < n)
    got = check(kset, D, n, max_dist, method=method)
    again = raw_closest(kset, n, max_dist, method=method)
    assert again[0] == 0 and all(np.array_equal(a.view(np.uint8), b.view(np.uint8)) for a, b in zip(got, again[1:]))


def test_method_auto_and_python_api(kset):
    import gdist
    D = R.recipe()[3]
    idx, d, cnt = check(kset, D, 10, 0.9, method=0)
    pidx, pd, pcnt = kset.closest(10, 0.9)
    assert pidx.shape == (N, 10) and pidx.dtype == np.int64 and pd.dtype == np.float64 and pcnt.dtype == np.int32
    assert np.array_equal(pidx, idx) and np.array_equal(pd.view(np.uint64), d.view(np.uint64))
    assert np.array_equal(pcnt, cnt)
    assert kset.getClosest(10, 0.9) == R.as_lists(idx, d, cnt)
    assert kset.getClosest(3, 0.9, rows=(3, 9), keep_self=True, method=gdist.METHOD_SORTED) == \
        R.as_lists(*R.closest_ref(D[3:9], 3, 0.9, r0=3, keep_self=True))


@pytest.mark.parametrize("method", [1, 2], ids=["sorted", "bitset"])
@pytest.mark.parametrize("rows_,cols_", [(7, 33), (64, 100), (128, 193), (1, 64)])
def test_chunking(kset, opts, method, rows_, cols_):
    """Several row blocks and column chunks with a ragged last chunk: the
    answer does not depend on closest_rows / closest_cols. At max_dist 1.0
    every row's tie group at 1.0 is longer than a chunk and n = 65 cuts it."""
    D = R.recipe()[3]
    assert N % cols_ != 0 and N > cols_
    below = ((D < 1.0) & ~np.eye(N, dtype=bool)).sum(1)
    assert (below < 65).any() and (below > 65).any()      # n = 65 ends inside the 1.0 group of some rows
    opts(closest_rows=rows_, closest_cols=cols_)
    check(kset, D, 10, 0.9, method=method)
    check(kset, D, 65, 1.0, method=method)


def test_rectangles_and_self(kset, opts):
    D = R.recipe()[3]
    for method in (1, 2):
        check(kset, D, 10, 0.9, rows=(3, 77), cols=(50, 160), method=method)      # the rows' own columns inside
        check(kset, D, 10, 0.9, rows=(150, 195), cols=(0, 150), method=method)    # disjoint: M x N use
    opts(closest_rows=16, closest_cols=50)
    check(kset, D, 10, 1.0, rows=(3, 77), cols=(50, 160))
    opts(closest_rows=None, closest_cols=None)
    idx, d, cnt = check(kset, D, 3, 0.9, flags=KEEP_SELF)
    # a set is at 0.0 from itself and leads its list unless an exact duplicate
    # has a lower index: sets 150, 151 repeat set 5 and set 152 repeats set 77
    dups = {150: [5, 150, 151], 151: [5, 150, 151], 152: [77, 152]}
    for q in range(N - 2):
        assert d[q, 0] == 0.0
        if q in dups:
            assert idx[q, :len(dups[q])].tolist() == dups[q]
        else:
            assert idx[q, 0] == q
    assert idx[5].tolist() == [5, 150, 151] and d[5].tolist() == [0.0, 0.0, 0.0]
    assert idx[77, :2].tolist() == [77, 152]
    assert cnt[N - 2:].tolist() == [0, 0]                 # the empty sets: at 1.0 from everything, themselves included
    # without KEEP_SELF the duplicates remain, the set itself does not
    idx, d, cnt = check(kset, D, 3, 0.9)
    assert idx[5, :2].tolist() == [150, 151] and idx[150, :2].tolist() == [5, 151]


@pytest.mark.parametrize("flags", [0, EMPTY_NAN], ids=["default", "empty_nan"])
def test_empty_sets(kset, flags):
    """Two empty sets: at 1.0 from everything by default (listed from max_dist
    1.0 on), NaN from each other and themselves with EMPTY_NAN (never listed)."""
    _, off, codes, _ = R.recipe()
    _, D = oracle.matrix(off, codes, 0, N, 0, N, flags=flags)
    assert int(np.isnan(D).sum()) == (4 if flags else 0)
    for method in (1, 2):
        for max_dist in (1.0, 0.99):
            idx, d, cnt = check(kset, D, 10, max_dist, method=method, flags=flags)
            assert cnt[N - 2:].tolist() == ([10, 10] if max_dist == 1.0 else [0, 0])
        idx, d, cnt = check(kset, D, 200, 1.0, method=method, flags=flags | KEEP_SELF)
        assert cnt[N - 1] == (N - 2 if flags else N)


def test_protein(ctx):
    import gdist
    from gdist import synth
    prots = [bytes(r) for r in synth.genomes(60, 400, 0.1, 43, protein=True)]
    off, codes = oracle.pack(prots, 8, 1, 0)
    _, D = oracle.matrix(off, codes, 0, 60, 0, 60)
    c = _candidates(D, 0.97)
    assert (c >= 5).any()
    s = gdist.KmerSets.from_sequences(prots, 8, gdist.KmerType.PROT, 0, ctx)
    for method in (1, 2):
        check(s, D, 5, 0.97, method=method)
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
    for n in (1, 10, 130):
        check(sk, D, n, 0.9, flags=flags)
        check(sk, D, n, 1.0, flags=flags)
    opts(closest_rows=50, closest_cols=37)
    check(sk, D, 10, 0.9, flags=flags)
    check(sk, D, 130, 1.0, flags=flags | KEEP_SELF)
    pidx, pd, pcnt = sk.closest(10, 0.9, rows=(100, 121), cols=(0, 100), flags=flags)
    assert R.as_lists(pidx, pd, pcnt) == R.as_lists(*R.closest_ref(D[100:121, 0:100], 10, 0.9, 100, 0))
    assert sk.getClosest(10, 0.9, rows=(100, 121), cols=(0, 100), flags=flags) == R.as_lists(pidx, pd, pcnt)


def test_errors_and_edge_cases(kset, ctx, sketch_case):
    import gdist
    from gdist import _lib as L
    D = R.recipe()[3]

    def einval(*a, **kw):
        rc, idx, d, cnt = raw_closest(*a, **kw)
        assert rc == L.EINVAL and L.lib.gdist_last_error()
        # refused before any work: the outputs keep the caller's values
        assert np.all(cnt == -9) and np.all(d == 7.5)

    einval(kset, 10, 0.9, rows=(0, N + 1))
    einval(kset, 10, 0.9, rows=(-1, 5))
    einval(kset, 10, 0.9, rows=(9, 5))
    einval(kset, 10, 0.9, cols=(0, N + 1))
    einval(kset, 10, 0.9, cols=(7, 3))
    einval(kset, 513, 0.9, rows=(0, 4))
    einval(kset, 10, float("nan"))
    einval(kset, 10, 0.9, flags=UPPER_TRIANGLE)
    einval(kset, 10, 0.9, flags=OUT_DEVICE)
    einval(kset, 10, 0.9, method=3)
    with pytest.raises(ValueError):
        kset.closest(-1, 0.9)
    idx, d, cnt = np.zeros(4, np.int64), np.zeros(4), np.zeros(2, np.int32)
    out = (L.ptr(idx, C.c_int64), L.ptr(d, C.c_double), L.ptr(cnt, C.c_int32))
    assert L.lib.gdist_closest(ctx.h, None, 0, 2, 0, 2, 0, 0, 2, 0.9, *out) == L.EINVAL      # null collection
    assert L.lib.gdist_closest(None, kset.h, 0, 2, 0, 2, 0, 0, 2, 0.9, *out) == L.EINVAL     # null context
    # a bitsets-only collection: SORTED is refused, BITSET and AUTO answer
    seqs = R.recipe_sequences()
    b = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    b.build_bitsets()
    b.release_codes()
    einval(b, 10, 0.9, method=1)
    check(b, D, 10, 0.9, method=2)
    check(b, D, 10, 0.9, method=0)
    b.free()
    # n = 0 and empty ranges: OK, counts 0
    rc, idx, d, cnt = raw_closest(kset, 0, 0.9)
    assert rc == 0 and np.all(cnt == 0) and idx.shape == (N, 0)
    rc, idx, d, cnt = raw_closest(kset, 10, 0.9, rows=(5, 5))
    assert rc == 0 and cnt.shape == (0,)
    rc, idx, d, cnt = raw_closest(kset, 4, 0.9, rows=(5, 9), cols=(20, 20))
    assert rc == 0 and np.all(cnt == 0) and np.all(idx == -1) and np.all(d == 1.0)
    pidx, pd, pcnt = kset.closest(0, 0.9)
    assert pidx.shape == (N, 0) and pd.shape == (N, 0) and np.all(pcnt == 0)
    # thresholds outside [0, 1]: nothing below a negative one, everything but NaN under +inf
    rc, idx, d, cnt = raw_closest(kset, 5, -1.0)
    assert rc == 0 and np.all(cnt == 0) and np.all(idx == -1) and np.all(d == 1.0)
    check(kset, D, 5, float("inf"))
    check(kset, D, 5, 0.0)                                   # exact duplicates only
    # sketches ignore the method argument
    sk, _ = sketch_case[64]
    a = raw_closest(sk, 5, 0.9, method=0)
    bb = raw_closest(sk, 5, 0.9, method=77)
    assert a[0] == 0 and bb[0] == 0 and all(np.array_equal(x, y) for x, y in zip(a[1:], bb[1:]))


def test_processor(ctx):
    """closest_genomes: the exact counterpart of the mash table
    (MashProcessor.java:144,161,168), text and counters from the oracle's matrix."""
    from gdist import processors
    from gdist.javafmt import java_format_f
    seqs, _, _, D = R.recipe()
    mk = lambda i: processors.Genome(f"83333.{i}", f"Genome number {i}", [seqs[i].decode()])
    subj_i = list(range(0, 120)) + [193]
    qry_i = [150, 136, 5, 160, 194, 147, 77, 152, 141]
    subjects, queries = [mk(i) for i in subj_i], [mk(i) for i in qry_i]
    sub = D[np.ix_(qry_i, subj_i)]
    eidx, ed, ecnt = R.closest_ref(sub, 10, 0.9, r0=len(subj_i), c0=0)
    assert (ecnt == 0).any() and (ecnt == 10).any() and ((ecnt > 0) & (ecnt < 10)).any()
    lines = ["query_id\tquery_name\tsubject_id\tsubject_name\tdistance"]
    for a, q in enumerate(queries):
        for r in range(ecnt[a]):
            s = subjects[eidx[a, r]]
            lines.append(f"{s.id}\t{s.name}\t{q.id}\t{q.name}\t{java_format_f(float(ed[a, r]), 8, 3)}")
    out = io.StringIO()
    counters = processors.closest_genomes(queries, subjects, out, ctx=ctx)
    assert out.getvalue() == "\n".join(lines) + "\n"
    assert counters == (len(queries), int(ecnt.sum()), int((ecnt == 0).sum()))
    assert "   0.000" in out.getvalue()                      # query 5 is subject 5: "%8.3f" of 0.0
    out = io.StringIO()
    assert processors.closest_genomes(queries[:2], subjects, out, neighbors=2, max_dist=0.5, ctx=ctx)[0] == 2
    e2 = R.closest_ref(sub[:2], 2, 0.5, r0=len(subj_i), c0=0)
    assert len(out.getvalue().splitlines()) == 1 + int(e2[2].sum())


def test_jni_closest(kset, tmp_path_factory):
    """nClosest through the shim equals the Python path; a null collection is
    an IllegalArgumentException."""
    from jni_harness import harness
    from jni_harness.harness import LONG, DOUBLE, INT
    jvm = harness.FakeJVM(harness.current() or
                          harness.build(str(tmp_path_factory.mktemp("jni") / "libgdist_jni_test.so")))
    seqs = R.recipe_sequences()
    sig = [C.c_int64] * 6 + [C.c_int32, C.c_int32, C.c_int32, C.c_double, C.c_void_p, C.c_void_p, C.c_void_p]
    ctx = jvm.call_i("nCtxCreate", C.c_int64, [C.c_int32], 0)
    sets = jvm.call_i("nPack", C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
                      ctx, 0, 21, 0, jvm.byte_arrays(seqs))
    assert jvm.exception() is None and sets
    for (r0, r1, c0, c1, n, md, fl) in ((0, N, 0, N, 10, 0.9, 0), (150, N, 0, 150, 65, 1.0, 0),
                                        (0, 20, 0, N, 3, 0.9, KEEP_SELF)):
        nr = r1 - r0
        ji, jd, jc = jvm.array(LONG, [7] * (nr * n)), jvm.array(DOUBLE, [7.5] * (nr * n)), jvm.array(INT, [-9] * nr)
        jvm.call_i("nClosest", None, sig, ctx, sets, r0, r1, c0, c1, 0, fl, n, md, ji, jd, jc)
        assert jvm.exception() is None
        pidx, pd, pcnt = kset.closest(n, md, rows=(r0, r1), cols=(c0, c1), keep_self=bool(fl))
        assert jvm.read(ji, LONG, nr * n) == pidx.ravel().tolist()
        assert np.array_equal(np.array(jvm.read(jd, DOUBLE, nr * n)).view(np.uint64), pd.ravel().view(np.uint64))
        assert jvm.read(jc, INT, nr) == pcnt.tolist()
    ji, jd, jc = jvm.zeros(LONG, 20), jvm.zeros(DOUBLE, 20), jvm.zeros(INT, 2)
    jvm.call_i("nClosest", None, sig, ctx, 0, 0, 2, 0, 2, 0, 0, 10, 0.9, ji, jd, jc)     # a null collection
    cls, msg = jvm.exception()
    assert cls == "java/lang/IllegalArgumentException" and msg
    jvm.call_i("nClosest", None, sig, ctx, sets, 0, 2, 0, 2, 0, 0, 10, 0.9, jvm.zeros(LONG, 19), jd, jc)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "idx shorter than (r1 - r0) * n")
    jvm.call_i("nClosest", None, sig, ctx, sets, 0, 2, 0, 2, 0, 0, 600, 0.9, jvm.zeros(LONG, 1200),
               jvm.zeros(DOUBLE, 1200), jc)
    assert jvm.exception()[0] == "java/lang/IllegalArgumentException"                     # n > GDIST_CLOSEST_MAX_N
    jvm.call("nFree", None, sets)
    jvm.call("nCtxDestroy", None, ctx)
    assert jvm.exception() is None
