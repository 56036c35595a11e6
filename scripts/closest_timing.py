"""Timing of the exact nearest-neighbour query (KmerSets.closest) on 4,096 DNA
genomes of 20 kbp (synth.genomes(4096, 20000, 0.02, 44), k = 21), n = 10,
max_dist = 0.9. One JSON line; each figure is the median of 5 runs after one
warm-up:

  a_closest_ms   KmerSets.closest over the full square, wall time
  b_matrix_ms    the route without it: matrix_device over row blocks of the same
                 size, D copied to the host, numpy top-n per row, wall time
  c_select_ms / c_matrix_ms
                 inside (a) with option time_kernels = 1: the select kernel alone
                 and the intersect kernels of the same blocks, HIP events on the
                 context's stream (Context.closest_timing)

The two routes' answers are compared (indices, fp64 bits, counts) before
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
    """matrix_device per row block, D to the host, numpy top-n per row."""
    idx = np.full((N, TOP), -1, dtype=np.int64)
    d = np.ones((N, TOP), dtype=np.float64)
    cnt = np.zeros(N, dtype=np.int32)
    cols = np.arange(N)
    for r0 in range(0, N, ROWS):
        r1 = min(N, r0 + ROWS)
        sets.matrix_device(None, dD.ptr, N, (r0, r1), (0, N))
        D = dD.to_host(np.float64, (r1 - r0) * N).reshape(r1 - r0, N)
        for a in range(r1 - r0):
            row = D[a]
            ok = row <= MAX_DIST
            ok[r0 + a] = False
            cand = np.flatnonzero(ok)
            take = cand[np.lexsort((cols[cand], row[cand]))][:TOP]
            cnt[r0 + a] = len(take)
            idx[r0 + a, :len(take)] = take
            d[r0 + a, :len(take)] = row[take]
    return idx, d, cnt


def median_ms(fn):
    fn()
    t = []
    for _ in range(RUNS):
        t0 = time.perf_counter()
        fn()
        t.append((time.perf_counter() - t0) * 1e3)
    return statistics.median(t)


def main():
    ctx = gdist.Context(0)
    g = synth.genomes(N, LENGTH, 0.02, 44)
    sets = gdist.KmerSets.from_sequences([bytes(r) for r in g], K, gdist.KmerType.DNA, 0, ctx)
    del g
    method = sets.prepare(gdist.METHOD_AUTO, float(N) * N)[0]
    dD = ctx.alloc(ROWS * N * 8)
    ctx.set_option("closest_rows", ROWS)
    got = sets.closest(TOP, MAX_DIST)
    exp = matrix_route(ctx, sets, dD)
    same = (np.array_equal(got[0], exp[0]) and np.array_equal(got[1].view(np.uint64), exp[1].view(np.uint64))
            and np.array_equal(got[2], exp[2]))
    if not same:
        raise SystemExit("closest and the matrix route disagree")
    a = median_ms(lambda: sets.closest(TOP, MAX_DIST))
    b = median_ms(lambda: matrix_route(ctx, sets, dD))
    ctx.set_option("time_kernels", 1)
    sets.closest(TOP, MAX_DIST)
    sel, mat = [], []
    for _ in range(RUNS):
        sets.closest(TOP, MAX_DIST)
        m, s = ctx.closest_timing()
        mat.append(m)
        sel.append(s)
    ctx.set_option("time_kernels", None)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    print(json.dumps({"config": f"{N} x {LENGTH} bp DNA, k={K}, n={TOP}, max_dist={MAX_DIST}, rows={ROWS}",
                      "method": {1: "sorted", 2: "bitset"}[method], "neighbours": int(got[2].sum()),
                      "a_closest_ms": round(a, 3), "b_matrix_ms": round(b, 3),
                      "c_select_ms": round(statistics.median(sel), 4),
                      "c_matrix_ms": round(statistics.median(mat), 4),
                      "commit": commit, "source_hash": _lib.lib.gdist_source_hash().decode()}))
    dD.free()
    sets.free()
    ctx.close()


if __name__ == "__main__":
    main()
