"""Every tuning option's values that no other test sets, bit-exact against
the oracle (include/gdist.h: "No option changes a result ... and the parity
tests run every non-default value against the oracle"). tests/option_cases.py
names, per option, the test that sweeps it; tests/test_option_table.py keeps
that table equal to GDIST_OPTIONS and checks that every `sweep` option is a
parameter id of this file.

Scene K: 300 x 20 kbp genomes (synth.genomes(300, 20000, 0.003, 11), DNA
k=21: the collection test_plan_follows_options shows to reach the sparse and
the rare tier; 300 is no multiple of a tile). Scene V: the c4_like recipe of
test_gpu_variant.py at its smallest size (300 sets, a forced variant tier).
Scene S: 50 uploaded sketches with the merge's edge cases. I is compared with
array_equal, D as uint64 views; no tolerance anywhere.

Each case asserts what the library can show of the code its option steers:
the info getters, the call's launch count and timing (a graph-replayed step
reports NaN times), the kernel families' event times under option
time_kernels, the sparse plan's chunk counts from option trace. Where the
library exposes nothing (the dense tiles' launch grouping and K split), the
case asserts this file's restatement of the launch arithmetic for its shapes
(so the shapes are known to meet the edge) and a comment names the source
line; such an assertion would not notice the library ignoring the option.
"""
import ctypes
import math
import os
import re

import numpy as np
import pytest

import oracle
from option_cases import SCENE_K, SCENE_S, SCENE_T

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
CSRC = os.path.join(ROOT, "genome.distance_amd", "csrc")

N = 300
CUS = 256                         # compute units of an MI355X (the gpu marker's device): ctx->cus
BT = 128                          # bitset_tiles.hpp: tile edge of the AND + popcount tiles
KC2 = 8                           # bitset.hip: words a chunk of those tiles
PARTIAL_MAX_RR = 6                # bitset_tiles.hpp: kPartialMaxRR
# (r0, r1, c0, c1, upper): the whole triangle, a row block that straddles the
# diagonal, a rectangle off every tile bound
REGIONS = [(0, 300, 0, 300, True), (129, 260, 0, 300, True), (37, 201, 5, 290, False)]
PAD = 7                           # device outputs: ld = nc + PAD
POISON_I, POISON_D = -7, 42.5
FAMILIES = ("sparse", "rare", "dense", "sorted", "variant")


def bits(a):
    return np.ascontiguousarray(a, np.float64).view(np.uint64)


# ---------------------------------------------------------------- scenes K and V
_SCENES = {}


def scene(name):
    """(sequences, the oracle's whole I, D), computed once a module."""
    if name not in _SCENES:
        from gdist import synth
        if name == "K":
            seqs = [bytes(r) for r in synth.genomes(N, 20000, 0.003, 11)]
        else:
            seqs = [bytes(r) for r in synth.genomes(1200, 4000, 0.03, 41)][:N]
        off, codes = oracle.pack(seqs, 21, 0, 0)
        eI, eD = oracle.matrix(off, codes, 0, N, 0, N, flags=0, nthreads=8)
        eI.setflags(write=False)
        eD.setflags(write=False)
        _SCENES[name] = (seqs, eI, eD)
    return _SCENES[name]


# what a scene is built with (options read at build time apply to collections
# built after the call: every case packs and builds after opts(...))
BASES = {
    # every dense word complement-sparse: the fused sparse step (tiles + reduce)
    "split": ("K", dict(sparse_zmax=100000)),
    # ... the rare pairs by the rare kernel, not the chunk reduce
    "split_rare": ("K", dict(sparse_zmax=100000, sparse_rare=0)),
    # sparse words beside dense words in their own tile launch (SPARSE_MODES
    # "mixed_tiles" of test_gpu_parity.py), the rare kernel on its own
    "mixed": ("K", dict(sparse_zmax=12, sparse_fold=0, sparse_rare=0)),
    # no sparse words: W = 640 dense words
    "dense": ("K", dict(sparse=0)),
    # ... 656 dense words: 82 chunks of 8, which 5 and 16 splits do not divide
    "dense82": ("K", dict(sparse=0, rare_t=3)),
    "variant": ("V", dict(variant=1, rare_t=3, variant_dmin=30)),
}


def build(ctx, opts, base, o):
    import gdist
    which, bo = BASES[base]
    seqs, eI, eD = scene(which)
    opts(**bo)
    opts(**o)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    ws, wd, _ = sets.sparse_info()
    nrare = sets.rare_info()[1]
    vk = sets.variant_info()[0]
    # the premises of the bases
    if base in ("split", "split_rare"):
        assert ws > 0 and wd == 0 and nrare > 0, (base, ws, wd, nrare)
    elif base == "mixed":
        assert ws > 0 and wd > 0 and nrare > 0, (base, ws, wd, nrare)
    elif base in ("dense", "dense82"):
        assert ws == 0 and wd == sets.bitset_info()[1] and nrare > 0, (base, ws, wd, nrare)
    else:
        assert vk > 0 and nrare > 0, (base, vk, nrare)
    return sets, eI, eD


def check_region(tag, I, D, eI, eD, r0, r1, c0, c1, up):
    xI, xD = eI[r0:r1, c0:c1], eD[r0:r1, c0:c1]
    if up:
        m = np.fromfunction(lambda a, b: (c0 + b) > (r0 + a), (r1 - r0, c1 - c0))
        I, D, xI, xD = I[m], D[m], xI[m], xD[m]
    assert np.array_equal(I, xI), (tag, r0, r1, c0, c1, up, np.flatnonzero(np.ravel(I != xI))[:5])
    assert np.array_equal(bits(D), bits(xD)), (tag, r0, r1, c0, c1, up)


def check_host_regions(tag, sets, eI, eD):
    import gdist
    for (r0, r1, c0, c1, up) in REGIONS:
        I, D = sets.matrix((r0, r1), (c0, c1), upper=up, method=gdist.METHOD_BITSET)
        check_region(tag, I, D, eI, eD, r0, r1, c0, c1, up)


def device_steps(tag, ctx, sets, eI, eD, calls=3, region=REGIONS[0]):
    """`region` (REGIONS[0]) into device outputs with ld > nc, `calls` times: the first
    call runs uncaptured, the second is captured, the rest replay the hipGraph.
    I and D are poisoned before the last call; after it the region's pairs
    equal the oracle and everything else (j <= i, the pad columns) is poison.
    Returns last_timing() after every call."""
    import gdist
    r0, r1, c0, c1, up = region
    nr, nc = r1 - r0, c1 - c0
    ld = nc + PAD
    dI, dD = ctx.alloc(nr * ld * 4), ctx.alloc(nr * ld * 8)
    timings = []
    try:
        dI.from_host(np.zeros(nr * ld, np.int32))
        dD.from_host(np.zeros(nr * ld))
        for call in range(calls):
            if call == calls - 1:
                dI.from_host(np.full(nr * ld, POISON_I, np.int32))
                dD.from_host(np.full(nr * ld, POISON_D))
            sets.matrix_device(dI.ptr, dD.ptr, ld, (r0, r1), (c0, c1), upper=up, method=gdist.METHOD_BITSET)
            timings.append(ctx.last_timing())
            I = dI.to_host(np.int32).reshape(nr, ld)
            D = dD.to_host(np.float64).reshape(nr, ld)
            check_region((tag, "device call", call), I[:, :nc], D[:, :nc], eI, eD, r0, r1, c0, c1, up)
        low = np.fromfunction(lambda a, b: (c0 + b) <= (r0 + a), (nr, nc))
        assert np.all(I[:, :nc][low] == POISON_I) and np.all(D[:, :nc][low] == POISON_D), (tag, "j <= i written")
        assert np.all(I[:, nc:] == POISON_I) and np.all(D[:, nc:] == POISON_D), (tag, "pad columns written")
    finally:
        dI.free()
        dD.free()
    return timings


def assert_replayed(tag, t):
    """The call replayed a captured step: one graph launch and, without option
    step_timing, no timing events (gdist.h: NaN times)."""
    k_ms, call_ms, launches = t
    assert launches == 1 and math.isnan(k_ms) and math.isnan(call_ms), (tag, t)


def family_ms(tag, ctx, opts, sets, eI, eD, region=REGIONS[0], method=None):
    """One more call over `region` under option time_kernels = 1 (HIP events
    around every kernel family's launches, no replay): exact, and the
    families' times, -1 for a family that did not run."""
    import gdist
    r0, r1, c0, c1, up = region
    opts(time_kernels=1)
    I, D = sets.matrix((r0, r1), (c0, c1), upper=up, method=gdist.METHOD_BITSET if method is None else method)
    ms = {f: ctx.kernel_ms(f) for f in FAMILIES}
    opts(time_kernels=None)
    check_region((tag, "time_kernels"), I, D, eI, eD, r0, r1, c0, c1, up)
    return ms


def assert_families(tag, ms, ran):
    for f in FAMILIES:
        if f in ran:
            assert ms[f] >= 0.0, (tag, f, ms)
        else:
            assert ms[f] == -1.0, (tag, f, ms)


def dense_launch_tiles(r0, r1, c0, c1, upper, split_diag, max_rr=PARTIAL_MAX_RR):
    """Tiles of the AND + popcount launches of a region, as matrix_plan groups
    them (matrix_step.hip, matrix_plan): off-diagonal, diagonal, partial off-diagonal, partial
    diagonal."""
    nr = r1 - r0
    tr = -(-nr // BT)
    corg = c0 - ((c0 - r0) % BT) if split_diag else c0
    dlt = (r0 - corg) // BT
    part = -(-(nr - (tr - 1) * BT) // 16) <= max_rr
    n = [0, 0, 0, 0]
    for a in range(tr):
        for b in range(-(-(c1 - corg) // BT)):
            rmin, cmax = r0 + a * BT, min(c1, corg + (b + 1) * BT) - 1
            if cmax < c0 or (upper and cmax <= rmin):
                continue
            n[(1 if split_diag and b - a == dlt else 0) + (2 if part and a == tr - 1 else 0)] += 1
    return n


def k_splits(tW, nt, wg_per_cu, min_chunks):
    """sp2 of one launch of nt tiles (bitset.hip, `launch` in dense_tiles_launch)."""
    nch2 = tW // KC2
    return max(1, min(max(1, nch2 // max(1, min_chunks)), -(-CUS * max(1, wg_per_cu) // nt)))


PLAN_LINE = re.compile(r"sparse chunks [a-z ()]+: (\d+) a tile \((\d+) on the diagonal\), (\d+) workgroups")


def plan_counts(err):
    """(chunks a tile, chunks a diagonal tile, workgroups) of every sparse plan
    option trace reported as built."""
    return [tuple(int(x) for x in m.groups()) for m in map(PLAN_LINE.search, err.splitlines()) if m]


# ---------------------------------------------------------------- scene K cases
# kind -> what the case asserts beyond exactness (below)
K_CASES = list(SCENE_K)


def case_id(base, o):
    return ",".join(f"{k}={v}" for k, v in o.items()) + "@" + base


def case_ids(o):
    return ",".join(f"{k}={v}" for k, v in o.items())


@pytest.mark.parametrize("base,o,kind", K_CASES, ids=[case_id(b, o) for b, o, _ in K_CASES])
def test_option_values_exact(ctx, opts, base, o, kind):
    """One row of option_cases.SCENE_K: the collection built under the
    options, three regions into host outputs, the first region three times
    into device outputs (uncaptured, captured, replayed into poisoned
    outputs), then once more under time_kernels; all exact, and the reach of
    the option asserted by `kind`."""
    tag = case_id(base, o)
    sets, eI, eD = build(ctx, opts, base, o)
    check_host_regions(tag, sets, eI, eD)
    t = device_steps(tag, ctx, sets, eI, eD)
    if kind == "no_graph":
        # gdist_api.hip, gdist_intersect_matrix: option graph = 0 takes neither
        # the capture nor the replay, every call records its timing events
        for k_ms, call_ms, launches in t:
            assert launches >= 1 and 0 < k_ms <= call_ms, (tag, t)
    else:
        assert_replayed(tag, t[-1])
    ms = family_ms(tag, ctx, opts, sets, eI, eD)
    ws, wd, _ = sets.sparse_info()
    W = sets.bitset_info()[1]
    if kind == "diag":
        # matrix_step.hip, matrix_plan: `split_diag = upper && bitset_diag != 0`;
        # 0 keeps corg = c0 and no DIAG group, so the diagonal tiles run in
        # the ordinary launch (with bitset_mfma default and >= 64 dense words
        # the MFMA tiles run instead and the option only moves the plan key)
        assert dense_launch_tiles(0, N, 0, N, True, False)[1::2] == [0, 0]
        assert dense_launch_tiles(0, N, 0, N, True, True)[1::2] == [2, 1]
        assert_families(tag, ms, {"dense", "rare"} | ({"sparse"} if ws else set()))
    elif kind.startswith("ksplit"):
        # bitset.hip, dense_tiles_launch `launch`: sp2 from bitset_wg_per_cu and
        # bitset_min_chunks over the launches of the whole triangle
        tW = wd if ws else W
        nch2 = tW // KC2
        assert tW % KC2 == 0 and nch2 == 82, (tag, tW)
        sp = [k_splits(tW, nt, o["bitset_wg_per_cu"], o["bitset_min_chunks"])
              for nt in dense_launch_tiles(0, N, 0, N, True, True) if nt]
        assert len(sp) == 3, (tag, sp)
        if kind == "ksplit_chunk":         # one 8-word chunk a workgroup
            assert all(x == nch2 for x in sp), (tag, sp)
        elif kind == "ksplit_one":         # no split
            assert all(x == 1 for x in sp), (tag, sp)
        else:                              # a last split shorter than the rest (or empty)
            assert all(1 < x < nch2 and nch2 % x != 0 for x in sp), (tag, sp)
        assert_families(tag, ms, {"dense", "rare"})
    elif kind == "partial":
        # matrix_step.hip, matrix_plan: `p.part = p.rr <= max_rr`. The whole
        # triangle's last row tile holds 44 rows (RR 3: launches of its own
        # unless bitset_partial_rr < 3); 240 rows leave 112 (RR 7: launches of
        # its own only with bitset_partial_rr 7)
        import gdist
        rr = o["bitset_partial_rr"]
        assert dense_launch_tiles(0, N, 0, N, True, True, rr)[2:] == ([0, 1] if rr >= 3 else [0, 0])
        assert dense_launch_tiles(0, 240, 0, N, True, True, rr)[2:] == ([1, 1] if rr >= 7 else [0, 0])
        assert dense_launch_tiles(0, 240, 0, N, True, True)[2:] == [0, 0]
        I, D = sets.matrix((0, 240), (0, N), upper=True, method=gdist.METHOD_BITSET)
        check_region(tag, I, D, eI, eD, 0, 240, 0, N, True)
        I, D = sets.matrix((7, 247), (3, 290), upper=False, method=gdist.METHOD_BITSET)
        check_region(tag, I, D, eI, eD, 7, 247, 3, 290, False)
        assert_families(tag, ms, {"dense", "rare"})
    elif kind == "order":
        # matrix_step.hip, bitset_matrix: `dense_first` decides whether
        # launch_side runs before or after the dense tiles' launch
        assert_families(tag, ms, {"dense", "rare"} | ({"sparse"} if ws else {"variant"}))
    elif kind == "summary":
        # bitset_build.hip, build_bitsets: `by_range = rs_opt > 0 || ...`: range_summary
        # instead of local_summary, at a size the default never takes it
        assert_families(tag, ms, {"sparse"})
    elif kind == "rare_inline":
        # matrix_step.hip, bitset_matrix: `overlap` / `rows_side` false, so the
        # rare kernel (list-major rare_pairs_kernel with rare_kernel 0, the
        # LDS-flushing rare_rows_kernel with 1) is issued on the main stream
        # after the join, with no fork of its own. The library cannot show
        # the stream: the launch count of 2 and the rare family's time only
        # show that the rare kernel ran apart from the sparse reduce, with
        # the option on or off. With sparse words and rare_kernel 1
        # `rows_side` is false whatever rare_overlap is (`!s->sparse`): that
        # case runs the row-major kernel in line, as the default would.
        assert ctx.last_timing()[2] == 2, (tag, ctx.last_timing())
        assert_families(tag, ms, {"rare", "sparse" if ws else "dense"})
    elif kind == "serial":
        # matrix_step.hip, bitset_matrix: `serial` puts launch_side on the main
        # stream (sd = st) ahead of the dense tiles and forces dense_first off
        side = {"sparse"} if ws else {"variant"}
        assert_families(tag, ms, {"dense", "rare"} | side)
    elif kind == "sparse_plan":
        # sparse.hip, sparse_plan: `target = cus x sparse_wg_per_cu`. At this
        # collection's ~626 sparse words the chunk count is bound by
        # ceil(Ws / 512) whatever the target, so these two cases only show
        # the sparse step exact with the option set; the counts that follow
        # the option are asserted by test_sparse_wg_per_cu_chunk_counts
        assert_families(tag, ms, {"sparse"})
    elif kind == "split_build":
        # bitset_build.hip, build_bitsets: range_summary = 0 asks for the one-sort summary;
        # a split build's shares are code ranges
        assert sets.build_timing()["shares"] == o["split_build"], (tag, sets.build_timing())
        assert_families(tag, ms, {"sparse"})
    elif kind == "no_graph":
        assert_families(tag, ms, {"sparse"})
    else:
        raise AssertionError(kind)
    sets.free()


# ---------------------------------------------------------------- sparse chunk counts
NW = 1200                         # scene W: 10 blocks of 128 sets, 55 tiles of the upper triangle
W_REGIONS = [(0, NW, 0, NW, True), (129, 1100, 0, NW, True)]


def scene_w():
    """1,200 x 8 kbp genomes of one ancestor (the c4_like recipe of
    test_gpu_variant.py at twice the length) and the oracle's upper triangle:
    with rare_t 3 every kmer of 3 or more sets is a dense-tier kmer, ~12,400
    words, all complement-sparse under sparse_zmax. ceil(Ws / 512) = 25 then
    exceeds cus x wg / 55 tiles for 1 and 4 workgroups a CU (5 and 19) and not
    for 16 (75): the three targets give three chunk counts."""
    if "W" not in _SCENES:
        from gdist import synth
        seqs = [bytes(r) for r in synth.genomes(NW, 8000, 0.03, 41)]
        off, codes = oracle.pack(seqs, 21, 0, 0)
        eI, eD = oracle.matrix(off, codes, 0, NW, 0, NW, flags=0x100, nthreads=16)
        eI.setflags(write=False)
        eD.setflags(write=False)
        _SCENES["W"] = (seqs, eI, eD)
    return _SCENES["W"]


@pytest.mark.parametrize("o", SCENE_T["test_sparse_wg_per_cu_chunk_counts"], ids=case_ids)
def test_sparse_wg_per_cu_chunk_counts(ctx, opts, capfd, o):
    """Option sparse_wg_per_cu on a collection whose sparse words outnumber
    the target's chunks (sparse.hip, sparse_plan: `target = cus x
    sparse_wg_per_cu`, n0 = min(ceil(Ws / 512), ceil(target / tiles)), then
    the taper's two rounds): the whole triangle's plan, as option trace prints
    it, holds fewer chunks a tile under 1 than under the default 4 and more
    under 16, and counts and distances stay exact over the triangle, a row
    block off the tile bounds, and three device steps (the last replayed into
    poisoned outputs)."""
    import gdist
    seqs, eI, eD = scene_w()
    opts(sparse_zmax=100000, rare_t=3)
    opts(**o)
    sets = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets()
    ws, wd, _ = sets.sparse_info()
    assert ws > 512 * 20 and wd == 0 and sets.rare_info()[1] > 0, (ws, wd, sets.rare_info())
    opts(trace=1)
    capfd.readouterr()
    for k, (r0, r1, c0, c1, up) in enumerate(W_REGIONS):
        I, D = sets.matrix((r0, r1), (c0, c1), upper=up, method=gdist.METHOD_BITSET)
        if k == 0:
            under = plan_counts(capfd.readouterr().err)
        check_region(o, I, D, eI, eD, r0, r1, c0, c1, up)
    # the same collection and region under the default target: another plan
    # key (matrix_step.hip, matrix_plan), so the plan is built and reported again
    opts(sparse_wg_per_cu=None)
    capfd.readouterr()
    I, D = sets.matrix(upper=True, method=gdist.METHOD_BITSET)
    default = plan_counts(capfd.readouterr().err)
    opts(trace=None)
    check_region("default target", I, D, eI, eD, 0, NW, 0, NW, True)
    assert under and default, (under, default)
    under, default = under[-1:], default[-1:]
    print(f"sparse chunks a tile: {o} {under[0]}, default {default[0]}")
    if o["sparse_wg_per_cu"] < 4:
        assert under[0][0] < default[0][0] and under[0][2] < default[0][2], (o, under, default)
    else:
        assert under[0][0] > default[0][0] and under[0][2] > default[0][2], (o, under, default)
    opts(**o)
    t = device_steps(o, ctx, sets, eI, eD, region=W_REGIONS[0])
    assert_replayed(o, t[-1])
    sets.free()


# ---------------------------------------------------------------- timing options
@pytest.mark.parametrize("o", SCENE_T["test_step_timing_of_replayed_steps"], ids=case_ids)
def test_step_timing_of_replayed_steps(ctx, opts, o):
    """Option step_timing = 1: a graph-replayed step records its timing
    events (finite 0 < kernel_ms <= call_ms, one launch); without it such a
    step reports NaN (gdist.h). Exact either way."""
    sets, eI, eD = build(ctx, opts, "split", {})
    t = device_steps("step_timing unset", ctx, sets, eI, eD)
    assert_replayed("step_timing unset", t[-1])
    opts(**o)
    t = device_steps("step_timing=1", ctx, sets, eI, eD)
    k_ms, call_ms, launches = t[-1]
    assert launches == 1 and math.isfinite(k_ms) and math.isfinite(call_ms) and 0 < k_ms <= call_ms, t
    sets.free()


@pytest.mark.parametrize("o", SCENE_T["test_time_kernels_matrix_families"], ids=case_ids)
def test_time_kernels_matrix_families(ctx, opts, o):
    """Option time_kernels = 1 on gdist_intersect_matrix (what the bench's
    roofline times family by family): exact results, gdist_ctx_kernel_ms >= 0
    for the families that ran and -1 for the others."""
    import gdist
    from gdist import _lib as L
    assert o == dict(time_kernels=1)          # family_ms sets it around its call
    sets, eI, eD = build(ctx, opts, "mixed", {})
    for region in REGIONS:
        ms = family_ms("time_kernels mixed", ctx, opts, sets, eI, eD, region)
        assert_families(("mixed", region), ms, {"sparse", "rare", "dense"})      # SORTED, VARIANT: -1
    ms = family_ms("time_kernels sorted", ctx, opts, sets, eI, eD, REGIONS[0], method=gdist.METHOD_SORTED)
    assert_families("sorted", ms, {"sorted"})
    # the device-output region under time_kernels: never replayed, timed every call
    opts(**o)
    t = device_steps("time_kernels device", ctx, sets, eI, eD)
    for k_ms, call_ms, launches in t:
        assert launches >= 1 and 0 < k_ms <= call_ms, t
    assert_families("device", {f: ctx.kernel_ms(f) for f in FAMILIES}, {"sparse", "rare", "dense"})
    opts(time_kernels=None)
    v = ctypes.c_double()
    assert L.lib.gdist_ctx_kernel_ms(ctx.h, len(FAMILIES), ctypes.byref(v)) != L.OK, "a family past the last"
    sets.free()
    vsets, vI, vD = build(ctx, opts, "variant", {})
    for region in REGIONS:
        ms = family_ms("time_kernels variant", ctx, opts, vsets, vI, vD, region)
        assert_families(("variant", region), ms, {"rare", "dense", "variant"})
    vsets.free()


def test_recent_timings_ring():
    """gdist_ctx_recent_timings on a context of its own: after k timed calls
    count == min(k, max), oldest first (each value is that call's
    last_timing kernel time: the same event pair), all > 0; max = 0 with a
    null buffer is accepted."""
    import gdist
    from gdist import _lib as L
    seqs, eI, eD = scene("K")
    c = gdist.Context(0)
    try:
        assert c.recent_timings(4) == []
        sets = gdist.KmerSets.from_sequences(seqs[:150], 21, gdist.KmerType.DNA, 0, c)
        sets.build_bitsets()
        seen = []
        for k, (r0, r1) in enumerate([(0, 150), (0, 1), (40, 150)], 1):
            I, D = sets.matrix((r0, r1), (0, 150), upper=True, method=gdist.METHOD_BITSET)
            check_region(("recent", k), I, D, eI, eD, r0, r1, 0, 150, True)
            seen.append(c.last_timing()[0])
            for mx in (1, 2, 3, 10):
                got = c.recent_timings(mx)
                assert len(got) == min(k, mx), (k, mx, got)
                assert got == seen[len(seen) - len(got):], (k, mx, got, seen)
                assert all(x > 0 for x in got), got
        cnt = ctypes.c_int(-1)
        L.check(L.lib.gdist_ctx_recent_timings(c.h, 0, None, ctypes.byref(cnt)))
        assert cnt.value == 0
        assert c.recent_timings(0) == []
    finally:
        c.close()


# ---------------------------------------------------------------- scene S
def _const(name):
    src = open(os.path.join(CSRC, "sketch.hip")).read()
    m = re.search(r"constexpr int %s = ([0-9* ]+);" % name, src)
    assert m, name
    v = 1
    for f in m.group(1).split("*"):
        v *= int(f)
    return v


def sketch_path(w, v2, k, only16):
    """The kernel sketch_matrix launches with sketch_phase = 0 (sketch.hip,
    launch_sketch_tiles): the 16 x 24 tile while its 40 sketches fit LDS, the
    16 x 16 tile while 32 do, else the global-memory form."""
    lds_max, slack = _const("LDS_SK_MAX"), _const("LDS_SK_SLACK")
    sw = ((w + 2) | 1) if (v2 and k == 2) else (w | 1)          # sketch_stride / the V2 rows' two sentinels

    def fits(ns):
        return ns * sw * 4 + slack + ns * (8 + 4) <= lds_max   # + sketch_meta_bytes

    if not only16 and fits(16 + 24):
        return "lds16x24"
    return "lds16x16" if fits(16 + 16) else "global"


_SKETCHES = {}


def sketches(w):
    """50 sketches of width w as test_sketch_merge_edges_vs_oracle builds
    them, and the oracle's (common, distance) of every pair for both flags."""
    import gdist
    if w not in _SKETCHES:
        rng = np.random.default_rng(1234 + w)
        sk = []
        for t in range(50):
            n = [0, 1, 2, w // 2, w - 1, w, w, w][t % 8]
            lo, hi = (-2**31, 2**31 - 1) if t % 3 else (-2**31, -2**31 + 40 * w)
            v = np.unique(rng.integers(lo, hi, size=3 * n + 8, endpoint=True, dtype=np.int64))
            v = np.sort(rng.choice(v, size=min(n, len(v)), replace=False)).astype(np.int32)
            if t % 11 == 0 and n:
                v[-1] = 2**31 - 1
                v = np.unique(v)
            if t % 13 == 0 and n:
                v[0] = -2**31
                v = np.unique(v)
            sk.append(v)
        sk[10] = sk[9].copy()                                     # identical pair
        sk[20] = np.arange(w, dtype=np.int32) * 2                 # disjoint interleaved pair
        sk[21] = np.arange(w, dtype=np.int32) * 2 + 1
        sk[30] = np.concatenate([[-2**31], sk[20][1:-1], [2**31 - 1]]).astype(np.int32)   # both ends
        assert {len(v) for v in sk} >= {0, 1, w - 1, w}
        ref = {}
        for fl in (0, gdist.SKETCH_JACCARD):
            eC = np.zeros((50, 50), np.int32)
            eD = np.zeros((50, 50))
            for i in range(50):
                for j in range(50):
                    eD[i, j], eC[i, j] = oracle.sketch_distance(sk[i], sk[j], w, fl)
            ref[fl] = (eC, eD)
        _SKETCHES[w] = (sk, ref)
    return _SKETCHES[w]


S_CASES = [(o, w, path) for (o, widths) in SCENE_S for (w, path) in widths]


@pytest.mark.parametrize("o,w,path", S_CASES,
                         ids=[",".join(f"{k}={v}" for k, v in o.items()) + f"@w{w}" for o, w, _ in S_CASES])
def test_sketch_tile_paths_exact(ctx, opts, o, w, path):
    """sketch_phase = 0 (whole sketches, not the ring kernel): the 16 x 16 LDS
    tile forced by sketch_tile = 16 at widths the 16 x 24 tile would take, the
    16 x 16 LDS tile at a width whose 40 sketches no longer fit LDS, and the
    global-memory form at a width whose 32 do not; each with sketch_v2 and the
    merge windows of sketch_k. Every pair of 50 sketches (no multiple of 16),
    both flags, against the oracle. The launch path follows from sketch.hip's
    LDS_SK_MAX and row stride (sketch_path): asserted per case."""
    import gdist
    only16 = o.get("sketch_tile") == 16
    v2, k = o.get("sketch_v2", 1) != 0, o.get("sketch_k", 2)
    assert sketch_path(w, v2, k, only16) == path, (o, w, sketch_path(w, v2, k, only16))
    if only16:
        assert sketch_path(w, v2, k, False) == "lds16x24", "only the option keeps the 16 x 24 tile away"
    sk, ref = sketches(w)
    opts(**o)
    S = gdist.SketchSets.from_signatures(sk, w, ctx)
    for fl in (0, gdist.SKETCH_JACCARD):
        C, D = S.matrix(flags=fl)
        # sketch.hip, sketch_matrix: `ring` false, one launch of the tiles
        assert ctx.last_timing()[2] == 1, ctx.last_timing()
        eC, eD = ref[fl]
        assert np.array_equal(C, eC), (o, w, fl, np.argwhere(C != eC)[:5])
        assert np.array_equal(bits(D), bits(eD)), (o, w, fl, np.argwhere(bits(D) != bits(eD))[:5])
        Cu, Du = S.matrix((3, 41), (1, 50), upper=True, flags=fl)
        m = np.fromfunction(lambda a, b: (1 + b) > (3 + a), (38, 49))
        assert np.array_equal(Cu[m], eC[3:41, 1:50][m]) and np.array_equal(bits(Du[m]), bits(eD[3:41, 1:50][m]))
    S.free()
