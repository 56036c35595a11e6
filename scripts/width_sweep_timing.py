"""Timing of the width processor's group step (processors.width_process_group)
by its two routes: one group of 1,000 synthetic proteins
(synth.genomes(1000, 400, 0.3, seed, protein=True), k = 8), sketch sizes
10 .. 390 step 10, the reference's defaults for the step and the group size.
One JSON line; --out PATH also writes it to a file.

  loop   sweep=False, the route of the parent commit and the baseline: the
         exact all-pairs once, then per size a sketch build, a sketch
         all-pairs, a download of the n x n doubles and the error in numpy
  sweep  sweep=True: one sketch build at the largest size and one
         KmerSets.width_sweep call (gdist_width_sweep)

Both in one process, alternated, one warm-up each and then RUNS repeats each:
wall time per group (host clock around the whole call; every route ends in a
download, so the device has finished), median and [min, max]. The lines the
two routes write are compared before anything is timed: group, size, pairs and
dwarves must be equal; lines whose printed mean or maximum differ are counted
(the sweep's total is the exact sum of the 2^-62-quantised errors, the loop's
the i-major fp64 sum)."""
import argparse
import io
import json
import os
import statistics
import subprocess
import sys
import time

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, os.path.join(ROOT, "genome.distance_amd"))

N, LENGTH, P_MAX, SEED, K = 1000, 400, 0.3, 14, 8
SIZES = list(range(10, 391, 10))
RUNS = 7


def stats(v):
    return {"median": round(statistics.median(v), 3), "min": round(min(v), 3), "max": round(max(v), 3)}


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--out", help="also write the JSON line to this file")
    ap.add_argument("--n", type=int, default=N, help="proteins in the group (a smaller one tries the script out)")
    args = ap.parse_args()
    import gdist
    from gdist import _lib, synth
    from gdist import processors as P
    ctx = gdist.Context(0)
    prots = [bytes(r) for r in synth.genomes(args.n, LENGTH, P_MAX, SEED, protein=True)]
    sets = gdist.KmerSets.from_sequences(prots, K, gdist.KmerType.PROT, 0, ctx)

    def run(sweep):
        out = io.StringIO()
        t = time.perf_counter()
        good = P.width_process_group("g", sets, SIZES, out, 0.001, sweep=sweep)
        ctx.synchronize()
        return (time.perf_counter() - t) * 1e3, good, out.getvalue().splitlines()

    # warm-up, and the two routes' lines against each other
    _, good_l, lines_l = run(False)
    _, good_s, lines_s = run(True)
    if len(lines_l) != len(lines_s) or len(lines_l) != len(SIZES):
        raise SystemExit("the routes wrote different numbers of lines")
    differ = 0
    for a, b in zip(lines_l, lines_s):
        fa, fb = a.split("\t"), b.split("\t")
        if fa[:4] != fb[:4]:
            raise SystemExit(f"the routes disagree: {a!r} / {b!r}")
        differ += fa[4:] != fb[4:]
    times = {"loop_ms": [], "sweep_ms": []}
    for _ in range(RUNS):
        times["loop_ms"].append(run(False)[0])
        times["sweep_ms"].append(run(True)[0])
    try:
        commit = subprocess.run(["git", "-C", ROOT, "rev-parse", "--short", "HEAD"], capture_output=True,
                                text=True).stdout.strip() or None
    except OSError:
        commit = None
    row = {"config": f"one group of {args.n} proteins of {LENGTH} aa (p_max {P_MAX}, seed {SEED}), k={K}, "
                     f"{len(SIZES)} sizes {SIZES[0]}..{SIZES[-1]} step 10; wall ms per group, median [min, max] of "
                     f"{RUNS} after a warm-up, routes alternated in one process",
           "pairs": int(lines_s[0].split("\t")[2]), "target_loop": good_l, "target_sweep": good_s,
           "lines_with_other_printed_error": int(differ)}
    row.update({k: stats(v) for k, v in times.items()})
    row["sweep_slowest_below_loop_fastest"] = bool(max(times["sweep_ms"]) < min(times["loop_ms"]))
    row["loop_over_sweep_median"] = round(statistics.median(times["loop_ms"]) / statistics.median(times["sweep_ms"]), 2)
    row["commit"] = commit
    row["source_hash"] = _lib.lib.gdist_source_hash().decode()
    line = json.dumps(row)
    print(line)
    if args.out:
        os.makedirs(os.path.dirname(os.path.abspath(args.out)), exist_ok=True)
        with open(args.out, "w") as f:
            f.write(line + "\n")
    sets.free()
    ctx.close()


if __name__ == "__main__":
    main()
