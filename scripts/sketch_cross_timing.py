"""Timing of query sketches against a resident sketch database
(SketchSets.cross_closest) on C5's sketches: 50,000 bottom-1000 MinHash
sketches of 100 kbp DNA genomes, k = 21, seeded as bench.py --config c5 builds
them (synth.genomes(.., 100000, 0.05, 5)); the queries are the next genomes of
the same series. n = 10, max_dist = 0.9, for Q = 1, 8, 64 and 1024 query rows
against all subjects. One JSON line.

Two routes in one process, alternated, a warm-up and then RUNS repeats each,
median and [min, max]:

  a  the cross call: subjects.cross_closest(queries) — wall time to the answer
     on the host, and with option time_kernels = 1 the merge kernel (join_ms)
     and the select kernel (select_ms) apart (Context.cross_info)
  b  the route before it: subjects.concat(queries) (a deep copy of the
     database), closest(rows = the queries, cols = the subjects, keep_self) on
     the copy — the concat's wall time, the closest's wall time, the two
     together, and the closest's matrix and select kernels (closest_timing)

Per Q also (subject bytes + query bytes) / join_ms as a share of the measured
HBM copy ceiling (6.29 TB/s, float4 copy): the bound of a route that reads
every subject once. `crossover_Q`: the first measured Q at which route b's
matrix kernel alone is faster than join_ms (null: none), for the follow-up that
sends wide rectangles through a two-source ring kernel.

The two routes' answers are compared (indices, fp64 bits, counts) before
anything is timed."""
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome.distance_amd"))
import numpy as np

N, LENGTH, P_MAX, CFG, K, WIDTH = 50000, 100_000, 0.05, 5, 21, 1000
TOP, MAX_DIST, RUNS = 10, 0.9, 7
QS = (1, 8, 64, 1024)
CHUNK = 512           # genomes a worker makes at a time; the smaller Q are heads of the first query chunk
COPY_CEILING = 6.29e12


def make_chunk(first, end):
    from gdist import synth
    return synth.to_blob(synth.genomes(min(CHUNK, end - first), LENGTH, P_MAX, CFG, first=first))


def stats(v):
    return {"median": round(statistics.median(v), 4), "min": round(min(v), 4), "max": round(max(v), 4)}


def same(x, y):
    return (np.array_equal(x[0], y[0]) and np.array_equal(x[1].view(np.uint64), y[1].view(np.uint64))
            and np.array_equal(x[2], y[2]))


def main():
    # SKETCH_CROSS_TIMING_N: a smaller database, for trying the script out
    n_subj = int(os.environ.get("SKETCH_CROSS_TIMING_N", "0")) or N
    import gdist
    from gdist import _lib
    ctx = gdist.Context(0)

    def sketched(blob, off):
        ks = gdist.KmerSets.from_blob(blob, off, K, gdist.KmerType.DNA, 0, ctx)
        try:
            return ks.sketches(WIDTH)
        finally:
            ks.free()

    def grown(old, sk):
        if old is None:
            return sk
        new = old.concat(sk)
        old.free()
        sk.free()
        return new

    t0 = time.perf_counter()
    subjects = None
    qsets = {}
    for first in range(0, n_subj, CHUNK):
        subjects = grown(subjects, sketched(*make_chunk(first, n_subj)))
    for first in range(N, N + max(QS), CHUNK):
        blob, off = make_chunk(first, N + max(QS))
        if first == N:
            for q in QS:
                if q < min(CHUNK, max(QS)):
                    qsets[q] = sketched(blob[:int(off[q])], off[:q + 1])
        qsets[max(QS)] = grown(qsets.get(max(QS)), sketched(blob, off))
    setup_s = time.perf_counter() - t0
    ns = len(subjects)
    sbytes = 4 * int(subjects.info()[3])

    rows = []
    for q in QS:
        queries = qsets[q]
        assert len(queries) == q

        def route_a():
            r = subjects.cross_closest(queries, TOP, MAX_DIST)
            ctx.synchronize()
            return r

        def route_b(times=None):
            t = time.perf_counter()
            both = subjects.concat(queries)
            ctx.synchronize()
            t1 = time.perf_counter()
            r = both.closest(TOP, MAX_DIST, rows=(ns, ns + q), cols=(0, ns), keep_self=True)
            ctx.synchronize()
            t2 = time.perf_counter()
            both.free()
            if times is not None:
                times["b_concat_ms"].append((t1 - t) * 1e3)
                times["b_closest_ms"].append((t2 - t1) * 1e3)
                times["b_total_ms"].append((t2 - t) * 1e3)
            return r

        ans = route_a()
        if not same(ans, route_b()):
            raise SystemExit(f"Q = {q}: the routes disagree")
        times = {k: [] for k in ("a_wall_ms", "b_concat_ms", "b_closest_ms", "b_total_ms")}
        for _ in range(RUNS):
            t = time.perf_counter()
            route_a()
            times["a_wall_ms"].append((time.perf_counter() - t) * 1e3)
            route_b(times)
        # the kernels apart
        ctx.set_option("time_kernels", 1)
        both = subjects.concat(queries)
        kt = {k: [] for k in ("join_ms", "select_ms", "b_matrix_ms", "b_select_ms")}
        units = 0
        for rep in range(RUNS + 1):
            subjects.cross_closest(queries, TOP, MAX_DIST)
            j, s, units = ctx.cross_info()
            both.closest(TOP, MAX_DIST, rows=(ns, ns + q), cols=(0, ns), keep_self=True)
            bm, bs = ctx.closest_timing()
            if rep:
                for k, v in zip(kt, (j, s, bm, bs)):
                    kt[k].append(v)
        both.free()
        ctx.set_option("time_kernels", None)
        nbytes = sbytes + 4 * int(queries.info()[3])
        jm = statistics.median(kt["join_ms"])
        row = {"Q": q, "units": int(units), "neighbours": int(ans[2].sum()), "bytes_read_once": nbytes,
               "join_share_of_copy_ceiling": round(nbytes / (jm * 1e-3) / COPY_CEILING, 4)}
        row.update({k: stats(v) for k, v in times.items()})
        row.update({k: stats(v) for k, v in kt.items()})
        row["a_below_b_spreads_apart"] = bool(max(times["a_wall_ms"]) < min(times["b_total_ms"]))
        rows.append(row)
        print(f"Q = {q}: a {row['a_wall_ms']['median']} ms, b {row['b_total_ms']['median']} ms", file=sys.stderr,
              flush=True)
    cross =[r["Q"] for r in rows if r["b_matrix_ms"]["median"] < r["join_ms"]["median"]]
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    print(json.dumps({"config": f"{ns} x bottom-{WIDTH} sketches of {LENGTH} bp DNA (k={K}, cfg {CFG}) resident, "
                                f"n={TOP}, max_dist={MAX_DIST}, median [min, max] of {RUNS} after a warm-up",
                      "setup_s": round(setup_s, 1), "rows": rows, "crossover_Q": cross[0] if cross else None,
                      "copy_ceiling_bytes_per_s": COPY_CEILING, "commit": commit,
                      "source_hash": _lib.lib.gdist_source_hash().decode()}))
    for h in list(qsets.values()) + [subjects]:
        h.free()
    ctx.close()


if __name__ == "__main__":
    main()
