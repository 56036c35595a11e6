"""Timing of the table-free queries of query batches against a resident
collection (KmerSets.cross_within, KmerSets.cross_histogram) on the collection
of scripts/cross_timing.py: 4,096 DNA genomes of 20 kbp (synth.genomes(4096,
20000, 0.02, 44), k = 21), batches of M = 1 and 16 mutated copies of subjects;
within at max_dist = 0.05, the histogram over the 50 buckets i / 50. One JSON
line. Per M and query, wall time from the batch's sequences to the answer on
the host, ending in a synchronise; the median of 5 after one warm-up, the
routes alternated within the one run:

  a_cross_ms    pack the batch, the cross call against the resident subjects
  c_concat_ms   pack the batch, subjects.concat(batch), the one-collection
                call (METHOD_SORTED, rows = the batch, cols = the subjects) on
                the copy

and, inside (a) with option time_kernels = 1 (Context.cross_info): the join
kernel and the consumer kernels (count + scan + write, or the histogram kernel;
HIP events, summed over the steps) and the work units.

The routes' answers are compared byte for byte before anything is printed."""
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

N, LENGTH, K, MAX_DIST, RUNS = 4096, 20000, 21, 0.05, 5
BATCHES = (1, 16)
EDGES = np.array([i / 50 for i in range(51)], dtype=np.float64)


def mutated(g, m, seed):
    """m rows of g (spread over the collection), 1 % of the positions replaced."""
    rng = np.random.default_rng(seed)
    rows = g[(np.arange(m) * (len(g) // m) + 7) % len(g)].copy()
    hit = rng.random(rows.shape) < 0.01
    rows[hit] = np.frombuffer(b"ACGT", dtype=np.uint8)[rng.integers(0, 4, int(hit.sum()))]
    return [bytes(r) for r in rows]


def main():
    ctx = gdist.Context(0)
    g = synth.genomes(N, LENGTH, 0.02, 44)
    subjects = gdist.KmerSets.from_sequences([bytes(r) for r in g], K, gdist.KmerType.DNA, 0, ctx)

    def cross(call):
        def route(batch):
            qs = subjects.pack_like(batch)
            r = call(qs)
            qs.free()
            ctx.synchronize()
            return r
        return route

    def concat(call):
        def route(batch):
            qs = subjects.pack_like(batch)
            both = subjects.concat(qs)
            r = call(both, len(batch))
            both.free()
            qs.free()
            ctx.synchronize()
            return r
        return route

    def within_bytes(r):
        return b"".join(x.tobytes() for x in r)

    queries = {
        "within": (cross(lambda qs: within_bytes(subjects.cross_within(qs, MAX_DIST))),
                   concat(lambda both, m: within_bytes(both.within(MAX_DIST, rows=(N, N + m), cols=(0, N),
                                                                   method=gdist.METHOD_SORTED, keep_self=True))),
                   lambda qs: subjects.cross_within(qs, MAX_DIST)),
        "histogram": (cross(lambda qs: subjects.cross_histogram(qs, EDGES).tobytes()),
                      concat(lambda both, m: both.histogram(EDGES, rows=(N, N + m), cols=(0, N), upper=False,
                                                            method=gdist.METHOD_SORTED).tobytes()),
                      lambda qs: subjects.cross_histogram(qs, EDGES)),
    }
    results = []
    for m in BATCHES:
        batch = mutated(g, m, 1000 + m)
        for name, (route_a, route_c, call) in queries.items():
            routes = (("a_cross_ms", route_a), ("c_concat_ms", route_c))
            ans = [fn(batch) for _, fn in routes]          # the warm-up, and the answers
            if ans[0] != ans[1]:
                raise SystemExit(f"M = {m}, {name}: the routes disagree")
            times = {r: [] for r, _ in routes}
            for _ in range(RUNS):
                for r, fn in routes:
                    t0 = time.perf_counter()
                    fn(batch)
                    times[r].append((time.perf_counter() - t0) * 1e3)
            row = {"query": name, "M": m}
            row.update({r: round(statistics.median(t), 3) for r, t in times.items()})
            # inside (a): the kernels apart
            ctx.set_option("time_kernels", 1)
            qs = subjects.pack_like(batch)
            join, sel, units = [], [], 0
            for rep in range(RUNS + 1):
                call(qs)
                j, s, units = ctx.cross_info()
                if rep:
                    join.append(j)
                    sel.append(s)
            qs.free()
            ctx.set_option("time_kernels", None)
            row.update({"join_ms": round(statistics.median(join), 4), "select_ms": round(statistics.median(sel), 4),
                        "units": int(units)})
            results.append(row)
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    print(json.dumps({"config": f"{N} x {LENGTH} bp DNA resident, k={K}, within max_dist={MAX_DIST}, histogram "
                                f"over {len(EDGES) - 1} buckets, median of {RUNS} after a warm-up",
                      "rows": results, "commit": commit, "source_hash": _lib.lib.gdist_source_hash().decode()}))
    subjects.free()
    ctx.close()


if __name__ == "__main__":
    main()
