"""Timing of the pairs-within-a-distance query (KmerSets.within) on 4,096 DNA
genomes of 20 kbp (synth.genomes(4096, 20000, 0.02, 44), k = 21), max_dist =
0.9: the collection of scripts/closest_timing.py. One JSON line; each figure is
the median of 5 runs after one warm-up:

  a_within_ms    KmerSets.within over the full square with the exact capacity,
                 wall time (a_count_ms: the counting call, capacity 0)
  b_matrix_ms    the route without it: matrix_device over row blocks of the same
                 size, D copied to the host, a numpy filter, wall time
  c_select_ms / c_matrix_ms
                 inside (a) with option time_kernels = 1: the count, scan and
                 write kernels and the intersect kernels of the same blocks, HIP
                 events on the context's stream (Context.within_timing);
                 c_count_only_ms: the same for the counting call;
                 low_select_ms: the same at low_max_dist, the 1 % quantile of the
                 distances (max_dist 0.9 passes every pair of this collection)
  closest_select_ms
                 the yardstick: the select kernel of closest(10, 0.9) in the same
                 process on the same collection (Context.closest_timing)

The two routes' answers are compared (row pointers, columns, fp64 bits) before
anything is printed."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome.distance_amd"))
import numpy as np

import gdist
from gdist import _lib, synth

N, LENGTH, K, TOP, MAX_DIST, ROWS, RUNS = 4096, 20000, 21, 10, 0.9, 4096, 5


def matrix_route(ctx, sets, dD):
    """matrix_device per row block, D to the host, numpy filter per block."""
    rowptr = np.zeros(N + 1, dtype=np.int64)
    cols, d = [], []
    for r0 in range(0, N, ROWS):
        r1 = min(N, r0 + ROWS)
        sets.matrix_device(None, dD.ptr, N, (r0, r1), (0, N))
        D = dD.to_host(np.float64, (r1 - r0) * N).reshape(r1 - r0, N)
        ok = D <= MAX_DIST
        ok[np.arange(r1 - r0), np.arange(r0, r1)] = False
        rowptr[r0 + 1:r1 + 1] = rowptr[r0] + np.cumsum(ok.sum(1))
        a, b = np.nonzero(ok)
        cols.append(b.astype(np.int64))
        d.append(D[a, b])
    return rowptr, np.concatenate(cols), np.concatenate(d)


def median_ms(fn):
    fn()
    t = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def timed(ctx, fn, read):
    fn()
    mat, sel = [], []
    for _ in range(RUNS):
        fn()
        m, s = read()
        mat.append(m)
        sel.append(s)
    return statistics.median(mat), statistics.median(sel)


def main():
    ctx = gdist.Context(0)
    g = synth.genomes(N, LENGTH, 0.02, 44)
    sets = gdist.KmerSets.from_sequences([bytes(r) for r in g], K, gdist.KmerType.DNA, 0, ctx)
    del g
    method = sets.prepare(gdist.METHOD_AUTO, float(N) * N)[0]
    dD = ctx.alloc(ROWS * N * 8)
    ctx.set_option("closest_rows", ROWS)
    got = sets.within(MAX_DIST)
    exp = matrix_route(ctx, sets, dD)
    same = (np.array_equal(got[0], exp[0]) and np.array_equal(got[1], exp[1])
            and np.array_equal(got[2].view(np.uint64), exp[2].view(np.uint64)))
    if not same:
        raise SystemExit("within and the matrix route disagree")
    total = int(got[0][-1])
    a = median_ms(lambda: sets.within(MAX_DIST, capacity=total))
    a0 = median_ms(lambda: sets.within(MAX_DIST, capacity=0))
    b = median_ms(lambda: matrix_route(ctx, sets, dD))
    ctx.set_option("time_kernels", 1)
    mat, sel = timed(ctx, lambda: sets.within(MAX_DIST, capacity=total), ctx.within_timing)
    _, cnt_only = timed(ctx, lambda: sets.within(MAX_DIST, capacity=0), ctx.within_timing)
    # a threshold that about 1 pair in 100 passes: the write kernel's share when few survive
    low = float(np.quantile(got[2], 0.01))
    low_total = int(sets.within(low, capacity=0)[0][-1])
    _, low_sel = timed(ctx, lambda: sets.within(low, capacity=low_total), ctx.within_timing)
    cmat, csel = timed(ctx, lambda: sets.closest(TOP, MAX_DIST), ctx.closest_timing)
    ctx.set_option("time_kernels", None)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    print(json.dumps({"config": f"{N} x {LENGTH} bp DNA, k={K}, max_dist={MAX_DIST}, rows={ROWS}",
                      "method": {1: "sorted", 2: "bitset"}[method], "pairs": total,
                      "a_within_ms": round(a, 3), "a_count_ms": round(a0, 3), "b_matrix_ms": round(b, 3),
                      "c_select_ms": round(sel, 4), "c_count_only_ms": round(cnt_only, 4),
                      "c_matrix_ms": round(mat, 4),
                      "low_max_dist": low, "low_pairs": low_total, "low_select_ms": round(low_sel, 4),
                      "closest_select_ms": round(csel, 4), "closest_matrix_ms": round(cmat, 4),
                      "commit": commit, "source_hash": _lib.lib.gdist_source_hash().decode()}))
    dD.free()
    sets.free()
    ctx.close()


if __name__ == "__main__":
    main()
