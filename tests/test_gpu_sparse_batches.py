"""Word batches of the sparse tile workgroups (options sparse_batch and
sparse_wtail). A workgroup's 8 waves deal the chunk's n words in batches of
48 words, a chunk of at most 8 x 48 words in equal shares of ceil(n / 8)
(sparse_batch absent or 0), or of a fixed 1..48 words (48: every chunk as
before this rule), and
a walk window's leftover groups of 64 slots go two to a step (sparse_wtail 1,
the default) or one at a time. Any partition of a chunk's words into batches
adds the same integers into the same counters, so every setting is bit-exact
against the oracle, I and D, over the whole upper triangle, a row-trimmed
block, a non-upper rectangle and the whole square, on the 300 sets of
test_gpu_sparse_balance (2 x 128 + 44: a partial last block).

The chunk counts are chosen from ws, the collection's sparse words, so that
the chunk sizes sit at the batch rule's edges; each premise is asserted from
ws and the chunk count of the plan's trace line."""
import re

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, LENGTH = 300, 20000
SNW, BATCH = 8, 48                        # waves a tile workgroup, most words a batch


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


_DATA = {}


def collection():
    """The sparse parity sweep's collection (300 x 20 kbp, p 0.003, seed 105)
    with the oracle's whole N x N matrices, computed once."""
    if not _DATA:
        from gdist import synth
        seqs = [bytes(r) for r in synth.genomes(N, LENGTH, 0.003, 105)]
        off, codes = oracle.pack(seqs, 21, 0, 0)
        eI, eD = oracle.matrix(off, codes, 0, N, 0, N, flags=0, nthreads=8)
        _DATA["base"] = (seqs, eI, eD)
    return _DATA["base"]


REGIONS = [(0, N, 0, N, True),            # the whole upper triangle
           (100, 250, 0, N, True),        # rows 100-250, upper
           (37, 211, 5, 290, False),      # a rectangle, not upper
           (0, N, 0, N, False)]           # the whole square


def check_regions(sets, eI, eD, tag):
    import gdist
    for (r0, r1, c0, c1, up) in REGIONS:
        I, D = sets.matrix((r0, r1), (c0, c1), upper=up, method=gdist.METHOD_BITSET)
        xI, xD = eI[r0:r1, c0:c1], eD[r0:r1, c0:c1]
        if up:
            mask = np.fromfunction(lambda a, b: (c0 + b) > (r0 + a), (r1 - r0, c1 - c0))
            I, D, xI, xD = I[mask], D[mask], xI[mask], xD[mask]
        assert np.array_equal(I, xI), (tag, r0, r1, c0, c1, up)
        assert bits_equal(D, xD), (tag, r0, r1, c0, c1, up)


PLAN = re.compile(r"sparse plan rows \[0,300\) cols \[0,300\): (\d+) tiles x (\d+) chunks, (partials|atomic flush)")
CHUNKS = re.compile(r"sparse chunks (balanced|balanced \(tapered\)|at equal counts): (\d+) a tile \((\d+) on the diagonal\)")


def plan_of(ctx, capfd, sets):
    """(kind, chunks a tile, chunks of a diagonal tile, partials or atomic
    flush) from the lines option trace prints when the whole triangle's plan
    is built."""
    import gdist
    capfd.readouterr()
    with ctx.options(trace=1):
        sets.matrix(upper=True, method=gdist.METHOD_BITSET)
    err = capfd.readouterr().err
    p = [m for m in map(PLAN.search, err.splitlines()) if m]
    c = [m for m in map(CHUNKS.search, err.splitlines()) if m]
    assert p and c, err[-2000:]
    assert int(p[-1].group(2)) == int(c[-1].group(2)), err[-2000:]
    return c[-1].group(1), int(c[-1].group(2)), int(c[-1].group(3)), p[-1].group(3)


def sizes_of(ws, nch):
    """The chunk sizes of nch chunks of equal word counts (bound c at
    ws c / nch, rounded down): ws / nch rounded down, and up unless it divides."""
    lo = ws // nch
    return {lo} if ws % nch == 0 else {lo, lo + 1}


def batch_of(n):
    """The rule's (rounds of 8 batches, batch words) of a chunk of n words."""
    rounds = -(-n // (SNW * BATCH))
    return rounds, (max(1, -(-n // SNW)) if rounds <= 1 else BATCH)


# name: (options of the plan as a function of ws, premise on (ws, kind, chunks, flush))
def _tiny(ws):
    return dict(sparse_balance=0, sparse_chunks=ws // 7 + 1)


def _tiny_ok(ws, kind, nch, flush):
    # every chunk under 8 words: batches of one word, waves with none
    return kind == "at equal counts" and all(0 < n < SNW and batch_of(n) == (1, 1) for n in sizes_of(ws, nch))


def _clip(target):
    def f(ws):
        # the first count from ws / target on whose chunks, all of 8..383
        # words, include one that is no multiple of 8
        nch = max(1, ws // target)
        while not any(n % 8 for n in sizes_of(ws, nch)):
            nch += 1
        return dict(sparse_balance=0, sparse_chunks=nch)
    return f


def _clip_ok(ws, kind, nch, flush):
    # one round whose 8 batches do not hold the same number of words: the
    # last waves' batches are shorter than the first's, or missing
    s = sizes_of(ws, nch)
    return (kind == "at equal counts" and all(8 <= n <= 383 and batch_of(n)[0] == 1 for n in s) and
            any(n % 8 and SNW * batch_of(n)[1] != n for n in s))


def _one(ws):
    return dict(sparse_chunks=1)


def _one_ok(ws, kind, nch, flush):
    # the whole list in one chunk: several rounds, flushed with atomics
    return nch == 1 and flush == "atomic flush" and batch_of(ws)[0] >= 2


def _two(ws):
    return dict(sparse_balance=0, sparse_chunks=ws // 385)


def _two_ok(ws, kind, nch, flush):
    # the most chunks that all hold more than 8 batches of 48: two rounds, the
    # waves claim their second batches from the LDS counter
    return kind == "at equal counts" and all(384 < n <= 768 and batch_of(n) == (2, BATCH) for n in sizes_of(ws, nch))


def _taper(ws):
    return {}


def _taper_ok(ws, kind, nch, flush):
    return kind == "balanced (tapered)" and nch > 1 and flush == "partials"


PLANS = {
    "tiny": (_tiny, _tiny_ok),
    "clip21": (_clip(21), _clip_ok),
    "clip100": (_clip(100), _clip_ok),
    "one": (_one, _one_ok),
    "two_rounds": (_two, _two_ok),
    "tapered": (_taper, _taper_ok),
}

# the kernel's settings run on every plan
VARIANTS = {
    "default": {},
    "batch48": dict(sparse_batch=48),
    "batch5": dict(sparse_batch=5),
    "batch1": dict(sparse_batch=1),
    "wtail0": dict(sparse_wtail=0),
    "wtail1": dict(sparse_wtail=1),
    "batch48_wtail0": dict(sparse_batch=48, sparse_wtail=0),      # the kernel before both
    "batch5_wtail0": dict(sparse_batch=5, sparse_wtail=0),
    "dyn0": dict(sparse_dyn=0),
    "dyn0_batch5": dict(sparse_dyn=0, sparse_batch=5),
    "dyn0_batch48_wtail0": dict(sparse_dyn=0, sparse_batch=48, sparse_wtail=0),
    "mt1": dict(sparse_mt=1),                                     # 1 x 2 micro-tiles, 4 groups a step
    "mt1_wtail0_batch5": dict(sparse_mt=1, sparse_wtail=0, sparse_batch=5),
    "atomic": dict(sparse_part_budget=0),
    "atomic_batch1": dict(sparse_part_budget=0, sparse_batch=1),
}


def run_variants(ctx, sets, eI, eD, tag, names=VARIANTS):
    for v in names:
        with ctx.options(**VARIANTS[v]):
            check_regions(sets, eI, eD, (tag, v))


@pytest.mark.parametrize("plan", list(PLANS))
def test_batches_exact(ctx, opts, capfd, plan):
    import gdist
    seqs, eI, eD = collection()
    opts(sparse_zmax=100000)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    ws, wd, ent = sets.sparse_info()
    assert ws > SNW * BATCH and wd == 0 and ent > 0, (ws, wd, ent)
    choose, premise = PLANS[plan]
    opts(**choose(ws))
    kind, nch, nd, flush = plan_of(ctx, capfd, sets)
    assert premise(ws, kind, nch, flush), (plan, ws, kind, nch, nd, flush)
    run_variants(ctx, sets, eI, eD, plan)
    sets.free()


@pytest.mark.parametrize("chunks", [2, 7, None])
def test_batches_folded_slabs(ctx, opts, chunks):
    """Dense words folded into the first chunks of every tile (their slab is
    staged in the record area after the waves' last batches)."""
    import gdist
    seqs, eI, eD = collection()
    opts(sparse_zmax=12, sparse_fold=100000)
    if chunks:
        opts(sparse_chunks=chunks)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    ws, wd, ent = sets.sparse_info()
    assert ws > 0 and wd > 0 and ent > 0
    run_variants(ctx, sets, eI, eD, ("slabs", chunks),
                 ("default", "batch48", "batch5", "batch1", "wtail0", "dyn0", "mt1", "atomic"))
    sets.free()


@pytest.mark.parametrize("chunks", [7, None])
def test_batches_automatic_tiers(ctx, opts, chunks):
    """The automatic choice of sparse words, with the rare tier (its rows are
    workgroups of the tile launch) and the group tier."""
    import gdist
    seqs, eI, eD = collection()
    if chunks:
        opts(sparse_chunks=chunks)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    assert sets.sparse_info()[0] > 0 and sets.rare_info()[1] > 0
    run_variants(ctx, sets, eI, eD, ("auto", chunks),
                 ("default", "batch48", "batch5", "batch1", "wtail0", "dyn0", "mt1", "atomic"))
    sets.free()


def test_batches_replayed_steps_poisoned(ctx, opts):
    """Four device-output calls over one region with the default options (the
    first builds the plan, the second is captured, the rest replay the graph)
    into outputs poisoned before every call: each equals the oracle over the
    region's upper triangle."""
    import gdist
    seqs, eI, eD = collection()
    opts(sparse_zmax=100000)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    for (r0, r1) in [(0, N), (100, 250)]:
        nr = r1 - r0
        mask = np.fromfunction(lambda a, b: b > (r0 + a), (nr, N))
        dI, dD = ctx.alloc(nr * N * 4), ctx.alloc(nr * N * 8)
        pI, pD = np.full(nr * N, -7, np.int32), np.full(nr * N, 42.5)
        for call in range(4):
            dI.from_host(pI)
            dD.from_host(pD)
            sets.matrix_device(dI.ptr, dD.ptr, N, (r0, r1), (0, N), upper=True, method=gdist.METHOD_BITSET)
            I = dI.to_host(np.int32).reshape(nr, N)
            D = dD.to_host(np.float64).reshape(nr, N)
            assert np.array_equal(I[mask], eI[r0:r1][mask]), (r0, call)
            assert bits_equal(D[mask], eD[r0:r1][mask]), (r0, call)
        dI.free()
        dD.free()
    sets.free()
