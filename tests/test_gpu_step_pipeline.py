"""Pipelined fused sparse steps: repeated matrix_device() calls over one plan
go out as direct launches on three streams, the tile kernel of call k + 1 on
its own stream into the plan's other copy of the chunk partials and the rare
slab, every reduce on the context's stream. What can go wrong
is ordering: a tile launch overwriting partials a reduce still reads, a tile
launch passing work queued on the context's stream before its call (uploads,
rebuilds, another collection's steps), outputs read before their reduce ran.

The scene is test_gpu_sparse_setup's: 300 sets in blocks of 128 + 128 + 44,
every word sparse, a rare tier present (its slab is the second buffer a step
owns). Calls come in bursts without a download or a synchronise between them;
after one synchronise I is compared exactly and D bit for bit, and every entry
a call must not write (j <= i of an upper region, the pad columns of
ld = nc + 3) still holds the poison. Context.step_info() tells which path ran;
the context is shared, so its counters are read as differences."""
import math

import numpy as np
import pytest

import oracle

pytestmark = pytest.mark.gpu

N, LENGTH = 300, 20000
PAD = 3
POISON_I, POISON_D = -7, 42.5
SLAB_TILE_BYTES = 128 * 128 * 4           # the rare slab: uint32 [tiles][128 x 128]

WHOLE = (0, N, 0, N, True)                # the whole upper triangle: 6 tiles
REGIONS = [WHOLE,
           (100, 250, 0, N, True),        # rows 100-250, upper: row-trimmed tiles
           (37, 211, 5, 290, False)]      # a rectangle, not upper
LAST_ROWS = (290, N, 0, N, True)          # ten rows of the last block: one short launch


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return np.array_equal(a.view(np.uint64), b.view(np.uint64))


def build(ctx, seqs):
    import gdist
    with ctx.options(sparse_zmax=100000):
        sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
        sets.build_bitsets()
    return sets


@pytest.fixture(scope="module")
def genomes():
    from gdist import synth
    return [bytes(r) for r in synth.genomes(N + 1, LENGTH, 0.003, 105)]


@pytest.fixture(scope="module")
def expected(genomes):
    """The oracle's whole I and D of the 300 sets, computed once."""
    from gdist import synth
    seqs = genomes[:N]
    assert seqs == [bytes(r) for r in synth.genomes(N, LENGTH, 0.003, 105)]   # the scene of test_gpu_sparse_setup
    off, codes = oracle.pack(seqs, 21, 0, 0)
    eI, eD = oracle.matrix(off, codes, 0, N, 0, N, flags=0, nthreads=8)
    eI.setflags(write=False)
    eD.setflags(write=False)
    return eI, eD


@pytest.fixture(scope="module")
def expected301(genomes):
    """The same for the 301 sets after one append, computed once."""
    off, codes = oracle.pack(genomes, 21, 0, 0)
    eI, eD = oracle.matrix(off, codes, 0, N + 1, 0, N + 1, flags=0, nthreads=8)
    eI.setflags(write=False)
    eD.setflags(write=False)
    return eI, eD


@pytest.fixture(scope="module")
def scene(ctx, genomes, expected):
    sets = build(ctx, genomes[:N])
    ws, wd, ent = sets.sparse_info()
    assert ws > 0 and wd == 0 and ent > 0, (ws, wd, ent)          # sparse words only
    assert sets.rare_info()[1] > 0                                 # a rare tier: the slab is in play
    out = Outputs(ctx, WHOLE)
    out.call(sets)
    assert ctx.last_timing()[2] == 1                               # the fused path
    out.check(expected, "fixture")
    out.free()
    yield sets
    sets.free()


class Outputs:
    """Device I and D of one region with ld = nc + 3, poisoned."""

    def __init__(self, ctx, region):
        self.ctx, self.region = ctx, region
        r0, r1, c0, c1, _ = region
        self.nr, self.nc = r1 - r0, c1 - c0
        self.ld = self.nc + PAD
        self.dI = ctx.alloc(self.nr * self.ld * 4)
        self.dD = ctx.alloc(self.nr * self.ld * 8)
        self.poison()

    def poison(self):
        self.dI.from_host(np.full(self.nr * self.ld, POISON_I, np.int32))
        self.dD.from_host(np.full(self.nr * self.ld, POISON_D))

    def call(self, sets, times=1):
        import gdist
        r0, r1, c0, c1, up = self.region
        for _ in range(times):
            sets.matrix_device(self.dI.ptr, self.dD.ptr, self.ld, (r0, r1), (c0, c1), upper=up,
                               method=gdist.METHOD_BITSET)

    def download(self):
        I = self.dI.to_host(np.int32).reshape(self.nr, self.ld)
        D = self.dD.to_host(np.float64).reshape(self.nr, self.ld)
        return I, D

    def check(self, exp, tag):
        """I exact, D bit for bit; what the call must not write holds the poison."""
        eI, eD = exp
        r0, r1, c0, c1, up = self.region
        I, D = self.download()
        mask = np.zeros((self.nr, self.ld), bool)
        mask[:, :self.nc] = (np.fromfunction(lambda a, b: (c0 + b) > (r0 + a), (self.nr, self.nc))
                             if up else True)
        xI = np.full((self.nr, self.ld), POISON_I, np.int32)
        xD = np.full((self.nr, self.ld), POISON_D)
        xI[:, :self.nc] = eI[r0:r1, c0:c1]
        xD[:, :self.nc] = eD[r0:r1, c0:c1]
        assert np.array_equal(I[mask], xI[mask]), (tag, self.region)
        assert bits_equal(D[mask], xD[mask]), (tag, self.region)
        assert np.all(I[~mask] == POISON_I) and np.all(D[~mask] == POISON_D), (tag, self.region)
        return I, D

    def free(self):
        self.dI.free()
        self.dD.free()


def delta(ctx, before):
    return tuple(a - b for a, b in zip(ctx.step_info(), before))


# 1 ---- a burst over one region ---------------------------------------------------------------
@pytest.mark.parametrize("region", REGIONS)
def test_burst(ctx, scene, expected, region):
    out = Outputs(ctx, region)
    s0 = ctx.step_info()
    out.call(scene, 2)
    s2 = ctx.step_info()
    out.call(scene, 4)
    ctx.synchronize()
    pipe, ordered, graph, held = delta(ctx, s0)
    assert pipe - ordered >= 4, (pipe, ordered)                  # calls 3-6 overlap their predecessors
    assert ctx.step_info()[1] == s2[1]                           # no fallback after the second call
    assert graph == 0
    assert ctx.step_info()[3] > 0
    assert ctx.last_timing()[2] == 1 and math.isnan(ctx.last_timing()[0])
    out.check(expected, "burst")
    out.free()


# 2 ---- two plans alternating, uneven load ----------------------------------------------------
def test_two_plans_alternating(ctx, scene, expected):
    """The ten-row launch runs beside the whole triangle's tail and ends first."""
    big, small = Outputs(ctx, WHOLE), Outputs(ctx, LAST_ROWS)
    s0 = ctx.step_info()
    for k in range(8):
        (small if k & 1 else big).call(scene)
    ctx.synchronize()
    pipe, ordered, graph, _ = delta(ctx, s0)
    assert pipe >= 4 and pipe - ordered >= 2 and graph == 0, (pipe, ordered, graph)
    big.check(expected, "big")
    small.check(expected, "small")
    big.free()
    small.free()


# 3 ---- something in between ------------------------------------------------------------------
def test_api_call_in_between_is_a_fallback(ctx, scene, expected):
    out = Outputs(ctx, WHOLE)
    out.call(scene, 3)
    s3 = ctx.step_info()
    out.poison()                                                 # gdist_memcpy_h2d: an API call
    out.call(scene)
    pipe, ordered, _, _ = delta(ctx, s3)
    assert (pipe, ordered) == (1, 1)
    out.call(scene, 2)
    assert delta(ctx, s3)[:2] == (3, 1)                          # and the run resumes
    ctx.synchronize()
    out.check(expected, "after from_host")
    out.free()


def test_append_in_between(ctx, genomes, expected, expected301, opts):
    """No tile launch after the append reads the 300 sets' entry arrays."""
    opts(sparse_zmax=100000)                                     # the rebuild keeps every word sparse
    sets = build(ctx, genomes[:N])
    out = Outputs(ctx, WHOLE)
    out.call(sets, 3)
    assert sets.append([genomes[N]]) == N
    out301 = Outputs(ctx, (0, N + 1, 0, N + 1, True))
    s0 = ctx.step_info()
    out301.call(sets, 4)
    ctx.synchronize()
    pipe, ordered, _, _ = delta(ctx, s0)
    assert pipe >= 2 and ordered >= 1, (pipe, ordered)
    assert sets.sparse_info()[1] == 0
    out.check(expected, "before the append")
    out301.check(expected301, "after the append")
    out.free()
    out301.free()
    sets.free()


# 4 ---- two collections on one context --------------------------------------------------------
def test_two_collections_alternating(ctx, scene, genomes, expected):
    other = build(ctx, genomes[:N])
    a, b = Outputs(ctx, WHOLE), Outputs(ctx, WHOLE)
    a.call(scene)
    b.call(other)
    s0 = ctx.step_info()
    for k in range(8):
        (b if k & 1 else a).call(other if k & 1 else scene)
    ctx.synchronize()
    pipe, ordered, graph, _ = delta(ctx, s0)
    assert pipe == 8 and ordered == 8 and graph == 0, (pipe, ordered, graph)
    a.check(expected, "first collection")
    b.check(expected, "second collection")
    a.free()
    b.free()
    other.free()


# 5 ---- serial_step = 1: the one-stream graph replay ------------------------------------------
@pytest.mark.parametrize("region", REGIONS)
def test_serial_step_replays_the_graph(ctx, scene, expected, opts, region):
    out = Outputs(ctx, region)
    out.call(scene, 6)
    ctx.synchronize()
    pI, pD = out.check(expected, "pipelined")
    out.poison()
    opts(serial_step=1)
    s0 = ctx.step_info()
    out.call(scene, 6)
    ctx.synchronize()
    pipe, ordered, graph, _ = delta(ctx, s0)
    assert pipe == 0 and ordered == 0 and graph >= 4, (pipe, ordered, graph)
    sI, sD = out.check(expected, "serial_step")
    assert np.array_equal(sI, pI) and bits_equal(sD, pD)
    out.free()


# 6 ---- no room for the second copies ---------------------------------------------------------
def test_budget_between_one_and_two_copies(ctx, scene, expected, opts):
    # a plan of this test's own (the option is in the plan's key) with room
    # for both copies: what it holds tells the size of one copy of the partials
    tiles = 6
    opts(sparse_part_budget=1 << 29)
    out = Outputs(ctx, WHOLE)
    s1 = ctx.step_info()
    out.call(scene, 4)
    ctx.synchronize()
    pipe, ordered, graph, held = delta(ctx, s1)
    one = held - tiles * SLAB_TILE_BYTES                         # 16-bit counters, 32 KiB a tile and chunk
    assert pipe >= 2 and one > 0 and one % (128 * 128 * 2) == 0, (pipe, held)
    out.check(expected, "with room")
    out.poison()
    opts(sparse_part_budget=one + one // 2)
    s2 = ctx.step_info()
    out.call(scene, 6)
    ctx.synchronize()
    pipe, ordered, graph, held = delta(ctx, s2)
    assert pipe == 0 and held == 0 and graph >= 4, (pipe, held, graph)
    out.check(expected, "one copy only")
    out.free()


# 7 ---- timed calls behind a pipelined burst --------------------------------------------------
def test_timed_calls_after_a_burst(ctx, scene, expected, opts):
    out = Outputs(ctx, WHOLE)
    out.call(scene, 5)
    opts(step_timing=1)                                          # no synchronise in between
    for _ in range(3):                                           # uncaptured, captured, replayed
        out.call(scene)
        k_ms, call_ms, launches = ctx.last_timing()
        assert launches == 1 and math.isfinite(k_ms) and k_ms > 0 and math.isfinite(call_ms), (k_ms, call_ms)
    out.check(expected, "step_timing")
    out.poison()
    opts(step_timing=None)
    out.call(scene, 5)
    opts(time_kernels=1)
    out.call(scene)
    k_ms, call_ms, _ = ctx.last_timing()
    assert math.isfinite(k_ms) and k_ms > 0 and math.isfinite(call_ms)
    assert math.isfinite(ctx.kernel_ms("sparse")) and ctx.kernel_ms("sparse") > 0
    out.check(expected, "time_kernels")
    out.free()
