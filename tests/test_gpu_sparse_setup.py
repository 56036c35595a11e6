"""The per-batch setup of the sparse tile workgroups: a wave takes the list
bounds of its batch's words once a lane in 32 bits (a word's lists end where
the next lane's start), sums the words' slot counts over its 64 lanes with DPP
adds (within rows of 16 lanes, then row 0 into row 1 and row 2 into row 3,
then rows 0-1 into rows 2-3) and claims its next batch from an LDS counter
that lane 0 reads for the wave.

The batch sizes put a batch's last word on and beside the rows' edges: lanes
15 | 16, 31 | 32 and 47 | 48 (48 words are the most a batch holds). A wrong
carry between two rows shifts the first slot of every later word of the
batch, a wrong end of a list changes a word's slot count: either way the
counters differ from the oracle's. The collection is test_gpu_sparse_batches'
(300 sets: blocks of 128 + 128 + 44, so that words without slots in the last
block's tiles sit between words with slots), every word sparse; I exactly and
D bit for bit over the whole upper triangle, a row-trimmed block, a non-upper
rectangle and the whole square."""
import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, LENGTH = 300, 20000
SNW = 8                                   # waves a tile workgroup

REGIONS = [(0, N, 0, N, True),            # the whole upper triangle
           (100, 250, 0, N, True),        # rows 100-250, upper
           (37, 211, 5, 290, False),      # a rectangle, not upper
           (0, N, 0, N, False)]           # the whole square

BATCHES = [15, 16, 17, 31, 32, 33, 47, 48]

# beside the batch size: the walk's modes and the ways a wave comes by its batches
VARIANTS = {
    "default": {},
    "dyn0": dict(sparse_dyn=0),                          # equal runs of words a wave, no claims
    "mt1": dict(sparse_mt=1),                            # 1 x 2 micro-tiles
    "diag22_0": dict(sparse_diag22=0),                   # diagonal tiles pair by pair
    "rpart22_0": dict(sparse_rpart22=0),                 # row-trimmed tiles in 1 x 2 micro-tiles
    "one_chunk_dyn0": dict(sparse_chunks=1, sparse_dyn=0),   # the atomic flush, several whole batches a wave
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
    # one chunk of all the words is several batches a wave at every batch size
    assert ws > SNW * max(BATCHES) and wd == 0 and ent > 0, (ws, wd, ent)
    yield sets, eI, eD
    sets.free()


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
@pytest.mark.parametrize("batch", BATCHES)
def test_setup_exact(ctx, scene, batch, variant):
    sets, eI, eD = scene
    with ctx.options(sparse_batch=batch, **VARIANTS[variant]):
        check_regions(sets, eI, eD, (batch, variant))
