"""The 3 x 3 walk of the sparse tile kernel (option sparse_mt 3, DESIGN.md
§4): off-diagonal tiles whose rows are not trimmed read triple records, three
entries of a (block, word) list in 32 bytes, a missing second or third entry
as word 0 / set 0, and form nine products a slot with no flag or count.

What can go wrong: a list's padding (n mod 3 = 1 or 2) counted as an entry or
an entry dropped, an empty list between lists with slots shifting the triple
offsets, the quotient of a slot by the column triples, the codes taken out of
a record's last two dwords, a tile that must keep the 2 x 2 walk (diagonal,
row-trimmed) reading triples. The collection is test_gpu_sparse_setup's (300
sets: blocks of 128 + 128 + 44, every word sparse): the 44-set block supplies
the empty and the short lists. I exactly and D bit for bit against the
oracle over that file's four regions, for sparse_mt 3 and — it has no other
default coverage now — sparse_mt 2."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, LENGTH = 300, 20000
PAD = 3
POISON_I, POISON_D = -7, 42.5

REGIONS = [(0, N, 0, N, True),            # the whole upper triangle
           (100, 250, 0, N, True),        # rows 100-250, upper: trimmed tiles (2 x 2) beside triple tiles
           (37, 211, 5, 290, False),      # a rectangle, not upper
           (0, N, 0, N, False)]           # the whole square

VARIANTS = {
    "default": {},
    "batch1": dict(sparse_batch=1),
    "batch15": dict(sparse_batch=15),
    "batch16": dict(sparse_batch=16),
    "batch17": dict(sparse_batch=17),
    "batch47": dict(sparse_batch=47),
    "batch48": dict(sparse_batch=48),
    "dyn0": dict(sparse_dyn=0),                          # equal runs of words a wave
    "wtail0": dict(sparse_wtail=0),                      # a window's leftover groups one at a time
    "one_chunk": dict(sparse_chunks=1),                  # the atomic flush
    "sun2": dict(sparse_sun=2),
    "sun3": dict(sparse_sun=3),
}


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


@pytest.fixture(scope="module")
def scene(ctx):
    """The collection with every word sparse, and the oracle's whole N x N I
    and D, computed once."""
    import gdist
    from gdist import synth
    seqs = [bytes(r) for r in synth.genomes(N, LENGTH, 0.003, 105)]
    off, codes = oracle.pack(seqs, 21, 0, 0)
    eI, eD = oracle.matrix(off, codes, 0, N, 0, N, flags=0, nthreads=8)
    eI.setflags(write=False)
    eD.setflags(write=False)
    with ctx.options(sparse_zmax=100000):
        sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
        sets.build_bitsets()
    ws, wd, ent = sets.sparse_info()
    assert ws > 0 and wd == 0 and ent > 0, (ws, wd, ent)
    yield sets, eI, eD
    sets.free()


def test_every_list_class_occurs(scene):
    sets, _, _ = scene
    ws, _, ent = sets.sparse_info()
    triples, empty, m1, m2, m0 = sets.sparse_triples()
    print(f"triples {triples}, lists: empty {empty}, n mod 3 = 1: {m1}, 2: {m2}, 0: {m0}; entries {ent}")
    assert min(empty, m1, m2, m0) > 0, (empty, m1, m2, m0)
    assert empty + m1 + m2 + m0 == 3 * ws                        # three blocks' lists of every sparse word
    assert 3 * triples - ent == 2 * m1 + m2, (triples, ent, m1, m2)


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


@pytest.mark.parametrize("variant", list(VARIANTS))
@pytest.mark.parametrize("mt", [3, 2])
def test_walk_exact(ctx, scene, mt, variant):
    sets, eI, eD = scene
    with ctx.options(sparse_mt=mt, **VARIANTS[variant]):
        check_regions(sets, eI, eD, (mt, variant))


@pytest.mark.parametrize("serial", [1, 0], ids=["replayed", "pipelined"])
def test_repeated_steps_poisoned(ctx, scene, opts, serial):
    """Device-output steps over the whole triangle into poisoned outputs with
    ld = nc + 3: replayed (serial_step 1: uncaptured, captured, two replays,
    poisoned before each) and pipelined (a burst of six with nothing between
    them, the last four overlapping their predecessors)."""
    import gdist
    sets, eI, eD = scene
    opts(sparse_mt=3, serial_step=serial)
    ld = N + PAD
    dI, dD = ctx.alloc(N * ld * 4), ctx.alloc(N * ld * 8)
    before = ctx.step_info()
    for k in range(4 if serial else 6):
        if serial or k == 0:
            dI.from_host(np.full(N * ld, POISON_I, np.int32))
            dD.from_host(np.full(N * ld, POISON_D))
        sets.matrix_device(dI.ptr, dD.ptr, ld, (0, N), (0, N), upper=True, method=gdist.METHOD_BITSET)
    ctx.synchronize()
    pipe, ordered, graph, _ = (a - b for a, b in zip(ctx.step_info(), before))
    assert (graph >= 2 and pipe == 0) if serial else (pipe - ordered >= 2 and graph == 0), (pipe, ordered, graph)
    I = dI.to_host(np.int32).reshape(N, ld)
    D = dD.to_host(np.float64).reshape(N, ld)
    mask = np.zeros((N, ld), bool)
    mask[:, :N] = np.triu(np.ones((N, N), bool), 1)
    assert np.array_equal(I[:, :N][mask[:, :N]], eI[mask[:, :N]])
    assert bits_equal(D[:, :N][mask[:, :N]], eD[mask[:, :N]])
    assert np.all(I[~mask] == POISON_I) and np.all(D[~mask] == POISON_D)
    dI.free()
    dD.free()
