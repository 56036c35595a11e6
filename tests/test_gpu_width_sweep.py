"""The sketch error at every sketch size in one walk of the pairs
(gdist_width_sweep; csrc/width_sweep.hip over the block walk, the lane-level
arithmetic in csrc/width_sweep.hpp). Every answer is compared with
width_sweep_ref (prefix signatures and distances of the oracle, Python-int
sums): `pairs` and every row field equal, the doubles as uint64 views. Both
flag values run everywhere. Outputs handed over through ctypes are pre-filled
with poison. The references are computed once a scene."""
import ctypes as C
import functools
import io
import struct

import numpy as np
import pytest

import pyref
import width_sweep_ref as R

pytestmark = pytest.mark.gpu

JACCARD = pyref.SKETCH_JACCARD
BOTH = (0, JACCARD)
AA = b"ACDEFGHIKLMNPQRSTVWY"


def proteins(n, length, rate, cfg):
    from gdist import synth
    return [bytes(r) for r in synth.genomes(n, length, rate, cfg, protein=True)]


def random_protein(seed, length):
    return bytes(np.random.default_rng(seed).choice(np.frombuffer(AA, np.uint8), length))


@functools.lru_cache(maxsize=None)
def scene(name):
    """name -> (sequences, k, kind)."""
    if name == "fam1":      # the width test's scene (test_gpu_parity.test_width_processor_vs_restatement)
        return proteins(14, 300, 0.10, 107), 8, pyref.PROT
    if name == "fam2":
        return proteins(11, 250, 0.30, 108), 8, pyref.PROT
    if name == "edges":
        # two identical proteins, one shorter than k (an empty set and signature), one with 5 kmers
        # (fewer than the smallest size), two that share nothing with anyone, and three relatives
        rel = proteins(3, 120, 0.15, 211)
        return ([rel[0], rel[0], b"ACDEF", rel[1][:12], random_protein(5, 90), random_protein(6, 90), rel[1], rel[2]],
                8, pyref.PROT)
    if name == "unrelated":  # no pair shares a kmer: every r is 1.0
        return [random_protein(20 + i, 80) for i in range(5)], 8, pyref.PROT
    if name == "n37":
        return proteins(37, 120, 0.25, 212), 8, pyref.PROT
    if name == "dna":       # sets of > 20,000 kmers: signatures that fill a width of 20,000
        from gdist import synth
        return [bytes(r) for r in synth.genomes(4, 14000, 0.02, 213)], 21, pyref.DNA
    raise KeyError(name)


@functools.lru_cache(maxsize=None)
def expected(name, sizes, flags, take=None):
    seqs, k, kind = scene(name)
    return R.expected(seqs[:take] if take else seqs, k, kind, sizes, flags)


@pytest.fixture(scope="module")
def device(ctx):
    """(name, take, width) -> (KmerSets, SketchSets) on the device, made on first use."""
    import gdist
    made = {}

    def get(name, width, take=None):
        key = (name, take, width)
        if key not in made:
            seqs, k, kind = scene(name)
            kt = gdist.KmerType.PROT if kind == pyref.PROT else gdist.KmerType.DNA
            sets = gdist.KmerSets.from_sequences(seqs[:take] if take else seqs, k, kt, 0, ctx)
            made[key] = (sets, sets.sketches(width))
        return made[key]
    yield get
    for sets, sk in made.values():
        sk.free()
        sets.free()


def dbits(x):
    return struct.unpack("<Q", struct.pack("<d", float(x)))[0]


def same(res, exp, tag=None):
    """A WidthSweep equals (pairs, rows) of the reference: integers equal, doubles bit for bit."""
    pairs, rows = exp
    assert res.pairs == pairs, (tag, res.pairs, pairs)
    assert len(res) == len(rows), tag
    for k, row in enumerate(rows):
        got = {"size": int(res.size[k]), "dwarves": int(res.dwarves[k]), "differing": int(res.differing[k]),
               "max_err": float(res.max_err[k]), "total": float(res.total[k]), "mean": float(res.mean[k]),
               "sum": res.sum[k]}
        for f in ("size", "dwarves", "differing", "sum"):
            assert got[f] == row[f], (tag, k, f, got[f], row[f])
        for f in ("max_err", "total", "mean"):
            assert dbits(got[f]) == dbits(row[f]), (tag, k, f, got[f], row[f])
        assert res.rows[k].pad == 0


# ---------------------------------------------------------------- 1. the width test's scene
@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("name", ["fam1", "fam2"])
def test_width_scene(device, name, flags):
    sizes = (20, 40, 60)
    sets, sk = device(name, 60)
    same(sets.width_sweep(sk, sizes, flags=flags), expected(name, sizes, flags), (name, flags))


# ---------------------------------------------------------------- 2. more than 64 and more than 128 sizes
@pytest.mark.parametrize("flags", BOTH)
def test_every_size_to_130(device, flags):
    sizes = tuple(range(1, 131))
    sets, sk = device("fam1", 130)
    same(sets.width_sweep(sk, sizes, flags=flags), expected("fam1", sizes, flags), flags)


def test_collection_wider_than_the_sizes(device):
    """The answer does not depend on the width sk was built at."""
    sizes = (20, 40, 60)
    sets, sk = device("fam1", 130)
    for flags in BOTH:
        same(sets.width_sweep(sk, sizes, flags=flags), expected("fam1", sizes, flags), flags)


# ---------------------------------------------------------------- 3. identical, empty, dwarf, disjoint
@pytest.mark.parametrize("flags", BOTH)
def test_edge_group(device, flags):
    sizes = (6, 20, 50)
    sets, sk = device("edges", 50)
    exp = expected("edges", sizes, flags)
    # what the scene is there for: a pair with r == s at every size (the identical two: both 0.0), pairs
    # with r == 1.0 that still differ from their sketch distance or not, dwarves at every size
    n = len(scene("edges")[0])
    assert exp[0] < n * (n - 1) // 2 and all(0 < r["differing"] < n * (n - 1) // 2 for r in exp[1])
    assert all(r["dwarves"] >= 2 for r in exp[1])
    same(sets.width_sweep(sk, sizes, flags=flags), exp, flags)


# ---------------------------------------------------------------- 4. one set, two sets
@pytest.mark.parametrize("flags", BOTH)
@pytest.mark.parametrize("n", [1, 2])
def test_one_and_two_sets(device, n, flags):
    sizes = (20, 40, 400)
    sets, sk = device("fam1", 400, take=n)
    res = sets.width_sweep(sk, sizes, flags=flags)
    same(res, expected("fam1", sizes, flags, n), (n, flags))
    if n == 1:
        assert res.pairs == 0 and not any(res.sum) and not res.differing.any()
    # no size at all: nothing to report
    none = sets.width_sweep(sk, (), flags=flags)
    assert none.pairs == 0 and len(none) == 0


# ---------------------------------------------------------------- 5. no pair below 1.0
@pytest.mark.parametrize("flags", BOTH)
def test_no_pair_below_one(device, flags):
    sizes = (10, 30)
    sets, sk = device("unrelated", 30)
    exp = expected("unrelated", sizes, flags)
    assert exp[0] == 0
    res = sets.width_sweep(sk, sizes, flags=flags)
    same(res, exp, flags)
    assert res.pairs == 0 and (res.mean == 0.0).all()


# ---------------------------------------------------------------- 6. block sizes
@pytest.mark.parametrize("cols", [16, 33])
@pytest.mark.parametrize("rows", [1, 16])
def test_block_sizes(device, opts, rows, cols):
    """Steps left of, on and right of the diagonal: the unblocked call's bytes."""
    sizes = (5, 17, 64)
    sets, sk = device("n37", 64)
    plain = {flags: sets.width_sweep(sk, sizes, flags=flags) for flags in BOTH}
    opts(closest_rows=rows, closest_cols=cols)
    for flags in BOTH:
        res = sets.width_sweep(sk, sizes, flags=flags)
        same(res, expected("n37", sizes, flags), (rows, cols, flags))
        assert res.tobytes() == plain[flags].tobytes()


# ---------------------------------------------------------------- 7. methods
def test_methods_agree(device):
    import gdist
    sizes = (5, 17, 64)
    sets, sk = device("n37", 64)
    for flags in BOTH:
        exp = expected("n37", sizes, flags)
        a = sets.width_sweep(sk, sizes, method=gdist.METHOD_SORTED, flags=flags)
        b = sets.width_sweep(sk, sizes, method=gdist.METHOD_BITSET, flags=flags)
        same(a, exp, ("sorted", flags))
        same(b, exp, ("bitset", flags))
        assert a.tobytes() == b.tobytes()


# ---------------------------------------------------------------- 8. the global-memory path
@pytest.mark.parametrize("flags", BOTH)
def test_wide_dna_sketches(device, flags):
    """Signatures of 20,000 hashes do not fit on chip: merged from global
    memory, and a lane's segment is longer than its 64-step mask."""
    sizes = (1, 64, 4097, 20000)
    sets, sk = device("dna", 20000)
    assert np.diff(sk.download()[0]).min() == 20000
    same(sets.width_sweep(sk, sizes, flags=flags), expected("dna", sizes, flags), flags)


# ---------------------------------------------------------------- 9. repeated and interleaved calls
def test_repeated_and_interleaved_calls(device):
    sizes = (5, 17, 64)
    sets, sk = device("n37", 64)
    for flags in BOTH:
        first = sets.width_sweep(sk, sizes, flags=flags).tobytes()
        assert sets.width_sweep(sk, sizes, flags=flags).tobytes() == first
        sk.matrix(upper=True)
        assert sets.width_sweep(sk, sizes, flags=flags).tobytes() == first


# ---------------------------------------------------------------- 10. EINVAL
def test_einval_leaves_outputs(ctx, device):
    import gdist
    from gdist import _lib as L
    sets, sk = device("fam1", 60)
    few, _ = device("fam1", 400, take=2)
    POISON = 0x5A

    def call(c=ctx.h, s=sets.h, k=sk.h, sizes=(20, 40, 60), method=0, flags=0, null_rows=False, null_pairs=False,
             null_sizes=False, nsizes=None):
        sz = np.asarray(sizes, dtype=np.int32)
        n = len(sz) if nsizes is None else nsizes
        rows = (L.WidthRow * max(len(sz), 1))()
        C.memset(rows, POISON, C.sizeof(rows))
        before = bytes(rows)
        pairs = C.c_int64(-77)
        rc = L.lib.gdist_width_sweep(c, s, k, n, None if null_sizes else L.ptr(sz, C.c_int32), method, flags,
                                     None if null_rows else C.addressof(rows), None if null_pairs else C.byref(pairs))
        return rc, bytes(rows) == before and pairs.value == -77

    assert call(c=None) == (L.EINVAL, True)
    assert call(s=None) == (L.EINVAL, True)
    assert call(k=None) == (L.EINVAL, True)
    assert call(null_rows=True) == (L.EINVAL, True)
    assert call(null_pairs=True) == (L.EINVAL, True)
    assert call(null_sizes=True) == (L.EINVAL, True)
    assert call(s=sk.h) == (L.EINVAL, True)                   # sets is a sketch collection
    assert call(k=sets.h) == (L.EINVAL, True)                 # sk is not one
    assert call(s=few.h) == (L.EINVAL, True)                  # 2 sets against 14 sketches
    assert call(sizes=(20, 20, 60)) == (L.EINVAL, True)       # not strictly increasing
    assert call(sizes=(40, 20, 60)) == (L.EINVAL, True)
    assert call(sizes=(0, 20, 60)) == (L.EINVAL, True)        # below 1
    assert call(sizes=(-5,)) == (L.EINVAL, True)
    assert call(sizes=(20, 40, 61)) == (L.EINVAL, True)       # above the width of sk
    assert call(nsizes=-1) == (L.EINVAL, True)
    assert call(nsizes=L.WIDTH_MAX_SIZES + 1) == (L.EINVAL, True)
    for flags in (L.EMPTY_NAN, L.UPPER_TRIANGLE, L.OUT_DEVICE, JACCARD | L.EMPTY_NAN, 0x1000):
        assert call(flags=flags) == (L.EINVAL, True), flags
    assert call(method=3) == (L.EINVAL, True)
    assert call(method=-1) == (L.EINVAL, True)
    other = gdist.Context(0)                                  # handles of another context
    fsets = gdist.KmerSets.from_sequences(scene("fam1")[0], 8, gdist.KmerType.PROT, 0, other)
    fsk = fsets.sketches(60)
    try:
        assert call(s=fsets.h) == (L.EINVAL, True)
        assert call(k=fsk.h) == (L.EINVAL, True)
        assert call(s=fsets.h, k=fsk.h) == (L.EINVAL, True)
        assert "another context" in L.lib.gdist_last_error().decode()
    finally:
        fsk.free()
        fsets.free()
    rc, clean = call()
    assert rc == 0 and not clean
    rc, clean = call(sizes=tuple(range(1, 61)))               # a full-length valid list
    assert rc == 0 and not clean
    with pytest.raises(ValueError):
        sets.width_sweep(sk, (20, 40), flags=L.EMPTY_NAN)
    with pytest.raises(ValueError):
        sets.width_sweep(sk, (2 ** 40,))


# ---------------------------------------------------------------- 11. the processor route
def processor_lines(ctx, sweep):
    from gdist import processors as P
    rows = [("fam1", s.decode()) for s in scene("fam1")[0]] + [("fam2", s.decode()) for s in scene("fam2")[0]]
    out = io.StringIO()
    target = P.width_processor(rows, 20, 60, out, step=20, max_group=12, target_error=0.05, kmer_size=8, ctx=ctx,
                               sweep=sweep)
    return out.getvalue().splitlines(), target


def test_processor_sweep_against_flat_route(ctx):
    flat, t_flat = processor_lines(ctx, False)
    sweep, t_sweep = processor_lines(ctx, True)
    assert sweep[0] == flat[0] == "Group\tSize\tPairs\tDwarves\tMean E\tMax E"
    assert len(sweep) == len(flat) == 1 + 3 * 3
    for a, b in zip(sweep[1:], flat[1:]):
        assert a.split("\t")[:4] == b.split("\t")[:4]
    assert t_sweep == t_flat


def test_processor_sweep_fields_against_reference(ctx):
    """Each mean and max-error field is the %8.4f of the reference row."""
    from gdist.javafmt import java_format_f
    sweep, _ = processor_lines(ctx, True)
    fam1, fam2 = scene("fam1")[0], scene("fam2")[0]
    exp = []
    for gid, prots in (("fam1", fam1[:12]), ("fam1", fam1[12:]), ("fam2", fam2)):
        pairs, rows = R.expected(prots, 8, pyref.PROT, (20, 40, 60), 0)
        assert pairs > 0
        for r in rows:
            exp.append(f"{gid}\t{r['size']:8d}\t{pairs:8d}\t{r['dwarves']:8d}\t{java_format_f(r['mean'], 8, 4)}\t"
                       f"{java_format_f(r['max_err'], 8, 4)}")
    assert sweep[1:] == exp
