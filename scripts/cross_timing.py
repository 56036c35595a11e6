"""Timing of query batches against a resident collection (KmerSets.cross_closest)
on 4,096 DNA genomes of 20 kbp (synth.genomes(4096, 20000, 0.02, 44), k = 21),
n = 10, max_dist = 0.9, for batches of M = 1, 16 and 256 mutated copies of
subjects. One JSON line. Per M, wall time from the batch's sequences to the
answer on the host, ending in a synchronise; the median of 5 after one warm-up,
the routes alternated within the one run:

  a_cross_ms    pack the batch, cross_closest against the resident subjects
  a2_copy_ms    the same against a device copy of the subjects (subjects.concat
                of an empty collection): a control, the same codes and the
                same segment index in another buffer
  b_repack_ms   the route of closest_genomes: pack subjects + batch as one
                collection, closest(rows = the batch, cols = the subjects)
  c_concat_ms   pack the batch, subjects.concat(batch), closest on the copy

and, inside (a) and (a2) with option time_kernels = 1 (Context.cross_info):
the join kernel and the select kernel (HIP events, summed over the steps), the
work units, and the join's achieved bytes / s: (query codes + streamed subject
codes) x 8 B over join_ms, next to the sorted join's model figure
kSortedBytesPerS (6.0e12, csrc/gdist_internal.hpp).

The routes' answers are compared (indices, fp64 bits, counts) before
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

N, LENGTH, K, TOP, MAX_DIST, RUNS = 4096, 20000, 21, 10, 0.9, 5
BATCHES = (1, 16, 256)
SORTED_BYTES_PER_S = 6.0e12


def mutated(g, m, seed):
    """m rows of g (spread over the collection), 1 % of the positions replaced."""
    rng = np.random.default_rng(seed)
    rows = g[(np.arange(m) * (len(g) // m) + 7) % len(g)].copy()
    hit = rng.random(rows.shape) < 0.01
    rows[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    return [bytes(r) for r in rows]


def same(x, y):
    return (np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64))
            and np.array_equal(x[2], y[2]))


def main():
    ctx = gdist.Context(0)
    g = synth.genomes(N, LENGTH, 0.02, 44)
    subj_seqs = [bytes(r) for r in g]
    subjects = gdist.KmerSets.from_sequences(subj_seqs, K, gdist.KmerType.DNA, 0, ctx)
    ssizes = subjects.sizes()
    none = subjects.pack_like([])
    copy = subjects.concat(none)
    none.free()

    def route_a(batch, resident=None):
        resident = resident or subjects
        qs = resident.pack_like(batch)
        r = resident.cross_closest(qs, TOP, MAX_DIST)
        qs.free()
        ctx.synchronize()
        return r

    def route_a2(batch):
        return route_a(batch, copy)

    def route_b(batch):
        both = gdist.KmerSets.from_sequences(subj_seqs + batch, K, gdist.KmerType.DNA, 0, ctx)
        r = both.closest(TOP, MAX_DIST, rows=(N, N + len(batch)), cols=(0, N))
        both.free()
        ctx.synchronize()
        return r

    def route_c(batch):
        qs = subjects.pack_like(batch)
        both = subjects.concat(qs)
        r = both.closest(TOP, MAX_DIST, rows=(N, N + len(batch)), cols=(0, N))
        both.free()
        qs.free()
        ctx.synchronize()
        return r

    routes = (("a_cross_ms", route_a), ("a2_copy_ms", route_a2), ("b_repack_ms", route_b), ("c_concat_ms", route_c))
    results = []
    for m in BATCHES:
        batch = mutated(g, m, 1000 + m)
        ans = [fn(batch) for _, fn in routes]          # the warm-up, and the answers
        if not all(same(ans[0], x) for x in ans[1:]):
            raise SystemExit(f"M = {m}: the routes disagree")
        times = {name: [] for name, _ in routes}
        for _ in range(RUNS):
            for name, fn in routes:
                t0 = time.perf_counter()
                fn(batch)
                times[name].append((time.perf_counter() - t0) * 1e3)
        row = {"M": m, "neighbours": int(ans[0][2].sum())}
        row.update({name: round(statistics.median(t), 3) for name, t in times.items()})
        # inside (a): the kernels apart
        ctx.set_option("time_kernels", 1)
        qs = subjects.pack_like(batch)
        qsizes = qs.sizes()
        join, sel, join2, units = [], [], [], 0
        for rep in range(RUNS + 1):
            subjects.cross_closest(qs, TOP, MAX_DIST)
            j, s, units = ctx.cross_info()
            copy.cross_closest(qs, TOP, MAX_DIST)
            j2 = ctx.cross_info()[0]
            if rep:
                join.append(j)
                sel.append(s)
                join2.append(j2)
        qs.free()
        ctx.set_option("time_kernels", None)
        blocks = -(-N // 64)
        codes = blocks * int(qsizes.sum()) + int((qsizes > 0).sum()) * int(ssizes.sum())
        jm, jm2 = statistics.median(join), statistics.median(join2)
        row.update({"join_ms": round(jm, 4), "select_ms": round(statistics.median(sel), 4), "units": int(units),
                    "join_bytes_per_s": round(codes * 8 / (jm * 1e-3), 0),
                    "join_vs_sorted_model": round(codes * 8 / (jm * 1e-3) / SORTED_BYTES_PER_S, 3),
                    "copy_join_ms": round(jm2, 4), "copy_join_bytes_per_s": round(codes * 8 / (jm2 * 1e-3), 0),
                    "copy_join_vs_sorted_model": round(codes * 8 / (jm2 * 1e-3) / SORTED_BYTES_PER_S, 3)})
        results.append(row)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    print(json.dumps({"config": f"{N} x {LENGTH} bp DNA resident, k={K}, n={TOP}, max_dist={MAX_DIST}, "
                                f"median of {RUNS} after a warm-up",
                      "batches": results, "commit": commit,
                      "source_hash": _lib.lib.gdist_source_hash().decode()}))
    copy.free()
    subjects.free()
    ctx.close()


if __name__ == "__main__":
    main()
