#!/usr/bin/env python3
"""Benchmark of the MI355X pairwise kmer-distance hot path (driver contract).

    python bench.py [--gpus N] [--steps K] [--warmup W] [--config c2|c2r|c3|c4|c5]
                    [--rows A:B] [--force-exchange] [--dump-outputs DIR] [--full]

A plain run sets up, warms up, times the K steps, writes the outputs if
--dump-outputs is given and prints the result line (metric, value,
ms_per_step, the workload and the setup times). --full goes on after the
timed steps with everything else: each kernel family timed alone and the
roofline built from it, the sample recount against poisoned outputs
(`verified`; a mismatch exits 1), the end-to-end figure and the CPU
baselines (--no-cpu-baseline leaves those out), and adds them to the line.
--dump-outputs DIR writes what the last timed step computed, this rank's
rows of I and D, as DIR/I.npy and DIR/D.npy (float64; see dump_outputs):
the inputs are generated from fixed seeds, so two builds can be compared
array for array.

Metric (BASELINE.json): genome-pair distances/sec over the N×N upper
triangle (unordered pairs i<j). Default workload = configs[1] (C2):
1,000 synthetic 2 Mbp genomes, DNA k=21 (both strands), dictionary-rank
bitsets, full N×N on one MI355X. A "step" is one pass of the hot path over
the resident packed sets: the tiled intersection kernel + the fp64 distance
epilogue into HBM (no D2H). Packing (FASTA bytes -> sorted codes ->
dictionary -> bitsets) happens once before timing and is reported as
`setup_s` fields, like the reference builds its kmer sets before the loop.

N>1 (torch.distributed.run, one process per GPU): weak scaling — the
genome count grows as 1000·sqrt(N) so every rank keeps ~C2's pair count;
each rank packs its own shard; the exchange is chosen by
gdist_sets_exchange_plan from its per-rank memory estimate: the dictionary
exchange (summaries, locus keys, bitsets, rare records; RCCL all-gathers)
when it fits, else ONE in-place all-gather of the packed codes for the
sorted join (C4: 100,000 x 100 kbp on 8 GPUs). Then every rank computes its
row block of the upper triangle; no collective in the timed region.
`value` = all ranks' pairs / max-over-ranks time.

--rows A:B (one GPU) times the rows [A, B) of the triangle only (a slice of
one rank's block, e.g. C4's per-rank workload); `value` is then the slice's
pairs / time and the line says so. --force-exchange runs the exchange on a
one-rank RCCL communicator (ncclAllGather on one GPU).

rank 0 prints one JSON line.
"""
from __future__ import annotations

import argparse
import json
import math
import os
import sys
import time

ROOT = os.path.dirname(os.path.abspath(__file__))
sys.path.insert(0, os.path.join(ROOT, "genome.distance_amd"))

import numpy as np  # noqa: E402

HBM_PEAK_GBS = 8000.0               # MI355X_MICROARCH.md chip table (spec)
# what bounds the sparse tile kernel (v6), from its PMC passes (profiles/r02/sparse6/)
SPARSE_LIMITER = ("latency of the product walk's scattered record loads, not HBM bandwidth or VALU issue: "
                  "a 2x2 micro-tile slot waits on four 12-16-byte record loads and adds four LDS counters "
                  "(VALU ~0.3 of its issue rate, TA ~0.5 busy, HBM traffic ~1.0x the algorithmic bytes; "
                  "DESIGN.md §4)")
# FP4 MFMA (block-scaled e2m1) dense peak, MI355X_MICROARCH.md chip table: ~10 PF
# dense = 5 P bit-products/s for the dense tiles on the matrix cores
MFMA_FP4_PEAK_TOPS = 10000.0
# VALU ceiling of the bitset inner step, MEASURED (scripts/microbench/valu_popc.hip,
# profiles/r01/valu_microbench.txt): an interleaved v_and_b32 + v_bcnt_u32_b32 stream
# issues at most 6.17e11 wave-instructions/s chip-wide (v_bcnt is half rate:
# 5.7e11 alone vs 1.06e12 for v_and). One 64-bit word pair = 4 wave-lane
# instructions (2 and + 2 bcnt) -> 6.17e11 * 64 / 4 word pairs/s.
VALU_WORDPAIR_PEAK = 6.17e11 * 64 / 4.0
# chip-wide VALU issue ceiling for plain 32-bit ops (v_and_b32 stream, same microbenchmark)
VALU_ISSUE_PEAK = 1.06e12
# LDS read peak for ds_read_b32-class reads (ds_read2_b32 banks as two of them):
# MI355X_MICROARCH.md §LDS, "≈75 TB/s for ds_read_b32" with every CU streaming.
LDS_B32_PEAK_GBS = 75000.0

CONFIGS = {
    # name: (n_genomes, length, p_max, kind, k, method, cfg index for the seed)
    "c2": dict(n=1000, length=2_000_000, p_max=0.002, protein=False, k=21, method="bitset", cfg=2,
               desc="1000 synthetic 2 Mbp genomes, DNA k=21 both strands, dictionary-rank bitsets"),
    "c2r": dict(n=1000, length=2_000_000, p_max=0.002, protein=False, k=21, method="bitset", cfg=2, realistic=True,
                desc="C2-realistic: 1000 synthetic ~2 Mbp genomes in 8 clades with short indels and segment "
                     "moves / inversions (gdist.synth.realistic_genome), DNA k=21 both strands, bitsets"),
    "c3r": dict(n=10000, length=33_333, p_max=0.10, protein=True, k=8, method="auto", cfg=3, realistic=True,
                desc="C3-realistic: 10000 synthetic ~33 kaa proteomes in 8 clades with short indels and segment "
                     "moves (gdist.synth.realistic_genome, protein), protein k=8, METHOD_AUTO"),
    "c4r": dict(n=100000, length=100_000, p_max=0.05, protein=False, k=21, method="auto", cfg=4, realistic=True,
                desc="C4-realistic: 100000 synthetic ~100 kbp genomes in 8 clades with short indels and segment "
                     "moves / inversions, DNA k=21 both strands, METHOD_AUTO (a one-GPU slice with --rows)"),
    "c3": dict(n=10000, length=33_333, p_max=0.10, protein=True, k=8, method="auto", cfg=3,
               desc="10000 synthetic 33,333-aa proteomes, protein k=8, sorted uint64 sets "
                    "(METHOD_AUTO: two-tier bitsets built from them, or the LDS hash-join)"),
    "c4": dict(n=100000, length=100_000, p_max=0.05, protein=False, k=21, method="auto", cfg=4,
               desc="100000 synthetic 100 kbp genomes, DNA k=21 both strands, row-sharded over 8 GPUs "
                    "(METHOD_AUTO; full size needs the 8-GPU node: use --n for a 1-GPU slice)"),
    "c5": dict(n=50000, length=100_000, p_max=0.05, protein=False, k=21, method="sketch", cfg=5, width=1000,
               desc="50000 MinHash bottom-1000 sketches of 100 kbp genomes (DNA k=21)"),
}


def log(*a):
    print(*a, file=sys.stderr, flush=True)


class stdout_to_stderr:
    """RCCL prints its version banner on stdout when a communicator is
    created; the driver reads ONE JSON line from stdout, so file descriptor
    1 points at stderr while the library initialises RCCL."""

    def __enter__(self):
        sys.stdout.flush()
        self.saved = os.dup(1)
        os.dup2(2, 1)

    def __exit__(self, *exc):
        sys.stdout.flush()
        os.dup2(self.saved, 1)
        os.close(self.saved)


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--gpus", type=int, default=1)
    ap.add_argument("--steps", type=int, default=50)
    ap.add_argument("--warmup", type=int, default=5)
    ap.add_argument("--config", default="c2", choices=sorted(CONFIGS))
    ap.add_argument("--n", "--genomes", dest="n", type=int, default=0,
                    help="override genome count (testing; --genomes under torch.distributed.run, whose own "
                         "options make --n ambiguous)")
    ap.add_argument("--length", type=int, default=0, help="override genome length (testing)")
    ap.add_argument("--method", default="", choices=["", "auto", "bitset", "sorted"],
                    help="override the config's kernel family (experiments; the config's own is the bench line)")
    ap.add_argument("--full", action="store_true",
                    help="after the timed steps also run what the headline figure does not need: per-kernel "
                         "timings and the roofline, the sample recount against poisoned outputs, the "
                         "end-to-end figure and the CPU baselines")
    ap.add_argument("--dump-outputs", default=None, metavar="DIR",
                    help="write the last timed step's outputs (this rank's rows of I and D) as DIR/<name>.npy")
    ap.add_argument("--no-cpu-baseline", action="store_true", help="with --full: leave the CPU baselines out")
    ap.add_argument("--pageable", action="store_true",
                    help="hand the pack the generated bytes in pageable memory instead of a gdist_host_alloc "
                         "buffer (the runtime's staged copies, ~6 GB/s)")
    ap.add_argument("--transport", default="rccl", choices=["rccl", "host"],
                    help="multi-rank exchange: RCCL (default) or host-staged over gloo (ranks sharing a GPU)")
    ap.add_argument("--same-device", action="store_true",
                    help="testing: every rank uses device 0 (rehearse the multi-rank path on one GPU)")
    ap.add_argument("--cpu-threads", type=int, default=0,
                    help="CPU baseline threads (default: this process's CPU share, see host_cpus())")
    ap.add_argument("--opt", action="append", default=[], metavar="NAME=VALUE",
                    help="context tuning option (gdist_ctx_set_option); GDIST_<NAME> variables are mapped too")
    ap.add_argument("--rows", default="", metavar="A:B",
                    help="one GPU: time rows [A, B) of the upper triangle only (a slice; the line reports it)")
    ap.add_argument("--force-exchange", action="store_true",
                    help="one GPU: run the multi-rank exchange on a one-rank RCCL communicator")
    ap.add_argument("--pmc-json", default=None,
                    help="per-launch HBM traffic measured by rocprofv3 PMC passes "
                         "(default: the profiles/pmc_<config>*.json taken on the line's kernel, if any)")
    args = ap.parse_args()
    if args.steps < 1 or args.warmup < 0:
        ap.error("--steps must be at least 1 and --warmup at least 0")

    rank = int(os.environ.get("RANK", "0"))
    world = int(os.environ.get("WORLD_SIZE", "1"))
    local_rank = int(os.environ.get("LOCAL_RANK", str(rank)))
    dist = None
    if world > 1:
        import torch.distributed as dist  # gloo: rendezvous, barrier, max over ranks
        dist.init_process_group("gloo", rank=rank, world_size=world)

    import gdist
    from gdist import shard, synth

    cfg = dict(CONFIGS[args.config])
    if args.n:
        cfg["n"] = args.n
    if args.length:
        cfg["length"] = args.length
    n_total = int(round(cfg["n"] * math.sqrt(world))) if world > 1 else cfg["n"]
    options = gdist.options_from_env()
    for kv in args.opt:
        k, v = kv.split("=", 1)
        options[k] = int(v)
    ctx = gdist.Context(0 if args.same_device else local_rank, options)

    def barrier():
        ctx.synchronize()
        if dist:
            dist.barrier()

    def max_over_ranks(v: float) -> float:
        if not dist:
            return v
        import torch
        t = torch.tensor([v], dtype=torch.float64)
        dist.all_reduce(t, op=dist.ReduceOp.MAX)
        return float(t.item())

    # ---------------------------------------------------------------- setup
    t_setup = time.time()
    s0, s1 = shard.shard_of_sets(n_total, world)[rank]
    t = time.time()
    if cfg.get("realistic"):
        rs = synth.realistic_genomes(s1 - s0, cfg["length"], cfg["p_max"], cfg["cfg"], first=s0,
                                     protein=cfg["protein"])
        blob = b"".join(rs)
        off = np.zeros(len(rs) + 1, dtype=np.int64)
        off[1:] = np.cumsum([len(x) for x in rs])
        del rs
    else:
        genomes = synth.genomes(s1 - s0, cfg["length"], cfg["p_max"], cfg["cfg"], protein=cfg["protein"], first=s0)
        blob, off = synth.to_blob(genomes)
        del genomes
    hostbuf = None
    if not args.pageable:
        # the FASTA bytes read into page-locked memory from gdist_host_alloc
        # (a reader fills it in place; here the generated bytes are copied
        # in, part of generation): the pack uploads it by DMA per chunk
        hostbuf = gdist.HostBuffer(len(blob))
        hostbuf.array[:] = np.frombuffer(blob, dtype=np.uint8)
        blob = hostbuf.array
    gen_s = time.time() - t
    kt = gdist.KmerType.PROT if cfg["protein"] else gdist.KmerType.DNA
    t = time.time()
    # the genomes as FASTA bytes in host memory: one buffer + offsets, handed
    # to gdist_sets_pack as they are (no per-genome copies)
    local = gdist.KmerSets.from_blob(blob, off, cfg["k"], kt, 0, ctx)
    pack_s = time.time() - t
    t = time.time()
    del blob                       # the caller's FASTA buffer (host page teardown, not pack work)
    if hostbuf is not None:
        hostbuf.free()
    free_s = time.time() - t
    t = time.time()
    method = args.method or cfg["method"]
    width_words = 0
    rare = None
    variant = None
    sparse_words = None
    auto = None
    exchange = world > 1 or args.force_exchange
    if exchange:
        if args.force_exchange and world == 1:
            with stdout_to_stderr():
                ctx.comm_init(gdist.Context.unique_id(), 1, 0)
            ctx.set_option("force_exchange", 1)
        elif args.transport == "host":
            import torch

            def gloo_allgather(a):
                t = torch.from_numpy(a)
                outs = [torch.empty_like(t) for _ in range(world)]
                dist.all_gather(outs, t)
                return torch.cat(outs).numpy()
            ctx.comm_init_host(world, rank, gloo_allgather)
        else:
            uid = gdist.Context.unique_id() if rank == 0 else None
            obj = [uid]
            dist.broadcast_object_list(obj, src=0)
            with stdout_to_stderr():
                ctx.comm_init(obj[0], world, rank)
    xplan = None
    build_t = None
    codes_gathered = False
    if exchange and method in ("auto", "bitset", "sorted"):
        # the exchange every rank takes (collective): the dictionary exchange
        # when its per-rank memory estimate fits, else the code all-gather
        # for the sorted join (gdist_sets_exchange_plan)
        want = {"auto": gdist.METHOD_AUTO, "bitset": gdist.METHOD_BITSET, "sorted": gdist.METHOD_SORTED}[method]
        m, bb, bc = local.exchange_plan(want)
        xplan = {"exchange": "bitsets" if m == gdist.METHOD_BITSET else "codes",
                 "est_bytes_per_rank": {"bitsets": bb if math.isfinite(bb) else None, "codes": bc}}
        if m == gdist.METHOD_BITSET:
            method = "bitset"
        else:
            # ONE code all-gather, consuming the local shard (peak (ranks + 1) x
            # shard); then METHOD_AUTO on the gathered collection priced on this
            # rank's block: the dictionary tiers built from the gathered codes
            # (C4: dense ancestral words + the variant tier), or the sorted join
            gathered = local.allgather(consume=True)
            if method == "sorted":
                local = gathered
            else:
                if args.rows:
                    a, b = (int(x) for x in args.rows.split(":"))
                else:
                    bnd = shard.triangle_bounds(n_total, world, 1)
                    a, b = bnd[rank], bnd[rank + 1]
                chosen, cb, cs = gathered.prepare(gdist.METHOD_AUTO, pairs=float(shard.pairs_in_rows(n_total, a, b)))
                auto = {"chosen": {gdist.METHOD_BITSET: "bitset", gdist.METHOD_SORTED: "sorted"}[chosen],
                        "est_bitset_s": round(cb, 4), "est_sorted_s": round(cs, 4), "after": "code all-gather"}
                method = auto["chosen"]
                local = gathered
                if method == "bitset":
                    # the tiers are built (split by rank on a multi-rank
                    # communicator): the gathered codes are not read again
                    build_t = gathered.build_timing()
                    gathered.release_codes()
            codes_gathered = True            # the gathered collection is what the step reads
    elif method == "auto":
        # METHOD_AUTO's own decision on one GPU (gdist_sets_prepare)
        chosen, cb, cs = local.prepare(gdist.METHOD_AUTO)
        auto = {"chosen": {gdist.METHOD_BITSET: "bitset", gdist.METHOD_SORTED: "sorted"}[chosen],
                "est_bitset_s": round(cb, 4), "est_sorted_s": round(cs, 4)}
        method = auto["chosen"]
    if method == "bitset":
        sets = local.allgather_bitsets() if exchange and not codes_gathered else local
        if not exchange and auto is None:
            sets.build_bitsets()
        dict_size, width_words = sets.bitset_info()
        rare = dict(zip(("threshold", "lists", "records"), sets.rare_info()))
        rare["kmers"] = sets.rare_kmers()
        sparse_words = dict(zip(("sparse_words", "dense_words", "entries"), sets.sparse_info()))
        if sparse_words["sparse_words"]:
            sparse_words["products"] = sets.sparse_pairs()
        vinfo = sets.variant_info()
        variant = dict(zip(("kmers", "words", "entries", "products"), vinfo)) if vinfo[0] else None
        if variant:
            variant["word_kmers"], variant["member_bytes"], variant["row_weight_max"] = sets.variant_layout()
        mflag = gdist.METHOD_BITSET
    elif method == "sorted":
        # the code all-gather consumes the local shard: peak (ranks + 1) x shard
        sets = local.allgather(consume=True) if exchange and not codes_gathered else local
        mflag = gdist.METHOD_SORTED
    else:
        sk_local = local.sketches(cfg["width"])
        sets = sk_local.allgather() if exchange else sk_local
        mflag = None
    represent_s = time.time() - t
    barrier()
    setup_s = time.time() - t_setup

    N = n_total
    # exact rows balancing the cost model's per-block time (dense tiles by
    # area, the rare kernel each rank's block picks); equal area otherwise.
    # Rank 0 cuts, every rank uses its cut.
    bounds = shard.triangle_bounds(N, world, 1)
    if method == "bitset" and world > 1:
        obj = [shard.balanced_bounds(N, world, lambda a, b: sets.block_cost((a, b))[0]) if rank == 0 else None]
        dist.broadcast_object_list(obj, src=0)
        bounds = obj[0]
    r0, r1 = bounds[rank], bounds[rank + 1]
    slice_rows = None
    if args.rows:
        assert world == 1, "--rows is a one-GPU slice"
        a, b = (int(x) for x in args.rows.split(":"))
        assert 0 <= a < b <= N, "--rows outside the collection"
        r0, r1 = a, b
        slice_rows = [a, b]
    rows = r1 - r0
    pairs_rank = shard.pairs_in_rows(N, r0, r1)
    dI = ctx.alloc(max(rows, 1) * N * 4)
    dD = ctx.alloc(max(rows, 1) * N * 8)

    def step():
        if method == "sketch":
            sets.matrix_device(dI.ptr, dD.ptr, N, (r0, r1), (0, N), upper=True)
        else:
            sets.matrix_device(dI.ptr, dD.ptr, N, (r0, r1), (0, N), upper=True, method=mflag)

    # the first call builds the region's launch plans (tile lists, sparse
    # chunks, the tile map of the rare rows: geometry only) before it runs;
    # every step recounts every pair, the rare tier included. Timed on its own, it is
    # part of the one-pass end-to-end figure; the second call is captured
    first_call_s = None
    for w in range(args.warmup):
        if w == 0:
            barrier()
            t = time.perf_counter()
            step()
            barrier()
            first_call_s = time.perf_counter() - t
        else:
            step()
    barrier()
    t0 = time.perf_counter()
    for _ in range(args.steps):
        step()                       # device outputs: returns once queued
    barrier()
    elapsed = time.perf_counter() - t0
    elapsed_max = max_over_ranks(elapsed)
    pairs_all = N * (N - 1) // 2
    pairs_job = pairs_rank if slice_rows else pairs_all      # a slice's pairs are all this job computes
    value = pairs_job * args.steps / elapsed_max
    dumped = None
    if args.dump_outputs:
        dumped = dump_outputs(args.dump_outputs, dI, dD, N, r0, r1, rank, world)
    config = {"workload": f"{args.config}: {cfg['desc']}", "genomes": N, "genome_length": cfg["length"],
              "k": cfg["k"], "pairs_per_step": pairs_job, "parallelism": f"rows{world}",
              "slice_rows": slice_rows, "exchange": xplan,
              "bitset_words_per_set": width_words or None,
              "dictionary_size": (dict_size if method == "bitset" else None),
              "method": method, "auto": auto, "rare_tier": rare, "complement_sparse": sparse_words,
              "variant_tier": variant,
              "options": options or None}
    setup = {"generate": round(gen_s, 2), "host_free": round(free_s, 3), "pack": round(pack_s, 2),
             "represent": round(represent_s, 2), "total": round(setup_s, 2),
             "build": ({k: (round(v, 1) if isinstance(v, float) else v) for k, v in build_t.items()}
                       if build_t else None)}

    def teardown():
        if dist:
            dist.barrier()
            ctx.comm_destroy()
            dist.destroy_process_group()
        elif exchange:
            ctx.comm_destroy()

    if not args.full:
        # the plain run ends here: the headline figure, nothing measured beside it
        if rank == 0:
            print(json.dumps({
                "metric": "genome-pair distances/sec (N×N)",
                "value": round(value, 1),
                "unit": "pairs/s",
                "n_gpus": world,
                "steps": args.steps,
                "warmup": args.warmup,
                "ms_per_step": round(elapsed_max / args.steps * 1e3, 4),
                "higher_is_better": True,
                "scaling": "weak",
                "vs_baseline": None,
                "dtype": "u64" if method != "sketch" else "i32",
                "data": "synthetic (splitmix64 genomes, SURVEY 8d)",
                "config": config,
                "setup_s": setup,
                "dumped": dumped,
                "full": False,
            }), flush=True)
        teardown()
        return
    # Kernel times, after the timed region: replayed steps record no timing
    # events by default (they cost 13-18 us a step), so a short loop with
    # option step_timing = 1 reads the steps' HIP-event spans (on the
    # library's streams); each kernel family alone below (time_kernels = 1)
    kt = max(3, min(args.steps, 20))
    prev_st = ctx.option("step_timing")
    ctx.set_option("step_timing", 1)
    for _ in range(kt):
        step()
    kernel_ms = ctx.recent_timings(kt)
    ctx.set_option("step_timing", prev_st)
    # Each kernel family alone, after the timed region (roofline): HIP events
    # around its launches on the stream they run on (option time_kernels; such
    # calls run unreplayed, one event pair per family and call): the sparse
    # tile launch, the rare-tier kernel, the dense tiles, the sorted join
    fam_ms = {}
    if method in ("bitset", "sorted"):
        # each family ALONE (option serial_step: the side stream's families
        # run on the main stream in turn), so that a kernel's roofline is its
        # own launch time, not its time while sharing the CUs with another
        prev, prev_serial = ctx.option("time_kernels"), ctx.option("serial_step")
        ctx.set_option("time_kernels", 1)
        ctx.set_option("serial_step", 1)
        acc = {f: [] for f in ctx.KERNEL_FAMILIES}
        for it in range(max(3, min(args.steps, 20))):
            step()
            for f in acc:
                v = ctx.kernel_ms(f)
                if it > 0 and v > 0:                       # the first call builds nothing new, but warms
                    acc[f].append(v)
        ctx.set_option("time_kernels", prev)
        ctx.set_option("serial_step", prev_serial)
        fam_ms = {f: float(np.mean(v)) for f, v in acc.items() if v}
    sparse_k_ms = fam_ms.get("sparse")
    k_avg_ms = float(np.mean(kernel_ms)) if kernel_ms else 0.0
    # end to end: the whole job for one pass over the collection = pack +
    # represent (dictionary, bitsets / sketches) + one step, max over ranks
    one_pass_s = first_call_s if first_call_s is not None else elapsed / max(args.steps, 1)
    e2e_s = max_over_ranks(pack_s + represent_s + one_pass_s)
    first_call_s = max_over_ranks(first_call_s) if first_call_s is not None else None

    verified = verify_sample(cfg, method, N, r0, r1, dI, dD, max_over_ranks, step=step)
    out = None
    if rank == 0:
        # ---------------------------------------------------------------- roofline
        if method == "bitset":
            bytes_per_pair = 16.0 * width_words                  # 16·W per pair
        elif method == "sorted":
            bytes_per_pair = 16.0 * float(np.mean(sets.sizes()))    # 8(n_i+n_j)
        else:
            # the sketch kernels merge from LDS; each merge step reads 2 dwords
            # and a pair of full sketches takes exactly `width` steps (the merge
            # ends at taken == width), so 8*width B of LDS reads per pair;
            # HBM/L2 traffic is the windows' fill, ~1/10 of that
            bytes_per_pair = 8.0 * cfg["width"]
        algo_bytes = pairs_rank * bytes_per_pair

        def pmc_sq(kern):
            """Per-launch SQ / TA counters of `kern` (profiles/pmc_<config>_sq.json,
            scripts/pmc_sq_json.py) with the kernel variant they were taken on."""
            fn = os.path.join(ROOT, "profiles", f"pmc_{args.config}_sq.json")
            try:
                with open(fn) as f:
                    pmc = json.load(f)
            except Exception:
                return None
            pk = pmc.get("kernel", "")
            ok = pk.replace(" ", "") == kern.replace(" ", "") if "<" in kern else pk.startswith(kern)
            if pmc.get("config") == args.config and pmc.get("n") == N and ok:
                return pmc
            return None

        traffic_readings = {}

        def pmc_traffic(kern):
            """HBM bytes per launch of `kern` from the committed PMC passes
            (profiles/pmc_<config>*.json: FETCH_SIZE x F + WRITE_SIZE), only a
            summary taken on this kernel at this collection size — with a
            template instantiation named (`kern` holding '<'), only one taken
            on that instantiation. Both FETCH readings (x1: scattered record
            loads, x2: the guide's streaming correction) are kept in
            traffic_readings for the line."""
            import glob
            files = [args.pmc_json] if args.pmc_json else \
                sorted(glob.glob(os.path.join(ROOT, "profiles", f"pmc_{args.config}*.json")))
            for fn in files:
                try:
                    with open(fn) as f:
                        pmc = json.load(f)
                except Exception:
                    continue
                pk = pmc.get("kernel", "")
                ok = pk.split(" (")[0].replace(" ", "") == kern.replace(" ", "") if "<" in kern else pk.startswith(kern)
                if pmc.get("config") == args.config and pmc.get("n") == N and ok:
                    traffic_readings[kern] = {"x1": pmc.get("hbm_bytes_x1"), "x2": pmc.get("hbm_bytes_x2"),
                                              "used": pmc.get("correction", "").split(",")[0],
                                              "kernel": pk.split(" (")[0],
                                              "source": os.path.relpath(fn, ROOT)}
                    return pmc.get("hbm_bytes_per_launch")
            return None

        sparse = sparse_words if (method == "bitset" and sparse_words and sparse_words["sparse_words"] > 0) else None
        sk_whole = options.get("sketch_phase", 1) == 0
        valu_peak = VALU_WORDPAIR_PEAK * 4 / 1e12
        if sparse:
            # Complement-sparse dense tier: the step's work is
            # the sparse tile kernel's products over (128-set block, sparse word)
            # entry lists. Algorithmic bytes = what each launched tile must stream
            # once: its row block's and column block's entries (8 B complement
            # word + 1 B set) and their (block, word) offsets (2 x 8 B), one side
            # for a whole diagonal tile.
            mt = options.get("sparse_mt", 2)
            sun = options.get("sparse_sun", 3 if mt == 2 else 4)
            kinst = f"sparse_tile_kernel<{sun}, {mt}>"
            kname = (f"{kinst} ({'2x2' if mt == 2 else '1x2'} micro-tiles, the dense words folded in, the rare rows "
                     "trailing)")
            nb = -(-N // 128)
            side = sparse["entries"] / nb * 9.0 + sparse["sparse_words"] * 16.0
            algo_sparse = 0.0
            for A in range(r0 // 128, (r1 - 1) // 128 + 1):
                rmin = max(r0, A * 128)
                for B in range(nb):
                    if min(N, (B + 1) * 128) - 1 <= rmin:
                        continue
                    whole_diag = A == B and A * 128 >= r0 and min(N, (A + 1) * 128) <= r1
                    algo_sparse += side if whole_diag else 2.0 * side
            kms = sparse_k_ms if sparse_k_ms else k_avg_ms
            ach = algo_sparse / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
            # VALU-issue roofline: the kernel's VALU
            # wave-instructions per launch (committed SQ pass) over the chip's
            # measured issue rate, against the live kernel time; per 64 of the
            # walk's products (sum over sparse words of z (z - 1) / 2)
            sq = pmc_sq(kinst)
            valu_issue = None
            if sq and sparse.get("products"):
                c = sq["counters_per_launch"]
                valu = c.get("SQ_INSTS_VALU")
                if valu:
                    floor_ms = valu / VALU_ISSUE_PEAK * 1e3
                    valu_issue = {"valu_per_launch": valu, "products": sparse["products"],
                                  "valu_per_64_products": round(valu * 64 / sparse["products"], 2),
                                  "issue_floor_ms": round(floor_ms, 4),
                                  "frac": round(floor_ms / kms, 3) if kms > 0 else None,
                                  "peak_wave_instr_per_s": VALU_ISSUE_PEAK,
                                  "ta_busy_frac": (round(c["TA_TA_BUSY_sum"] / 256 / (c["GRBM_GUI_ACTIVE"] / 8), 3)
                                                   if c.get("TA_TA_BUSY_sum") and c.get("GRBM_GUI_ACTIVE") else None),
                                  "counters_from": sq.get("kernel"), "source": sq.get("source")}
            dense_ops = pairs_rank * width_words * 4 / (k_avg_ms * 1e-3) / 1e12 if k_avg_ms > 0 else 0.0
            roof = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                    "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": pmc_traffic(kinst),
                    "kernel": kname, "kernel_avg_ms": round(kms, 4), "step_kernel_span_ms": round(k_avg_ms, 4),
                    "algo_bytes_per_launch": round(algo_sparse),
                    "limiter": SPARSE_LIMITER,
                    "note": "algorithmic bytes = the sparse entries (8 B word + 1 B set) + offsets each sparse "
                            "tile streams once; kernel_avg_ms = HIP events around the sparse tile launch alone "
                            "(option time_kernels, after the timed region; its trailing workgroups recount the "
                            "rare tier's pairs of the step); step_kernel_span_ms = HIP-event span of the timed "
                            "steps' launches (sparse tiles + rare rows, then the chunk reduce that stores I and D)",
                    "valu_issue": valu_issue,
                    "dense_equivalent": {"lane_ops_per_s_T": round(dense_ops, 2),
                                         "x_dense_valu_ceiling": round(dense_ops / valu_peak, 2),
                                         "note": "the same pairs as AND+popcount over all W bitset words "
                                                 "(4 lane-ops per word pair) in the step's kernel time, against the "
                                                 "measured and+bcnt ceiling the dense tiles are bound by"}}
        elif method == "bitset":
            # Two tiers in one step (C3): the dense tiles (VALU-bound: they reuse
            # each bitset from LDS across 128 partners, so the 16*W B/pair
            # streaming figure runs far past the HBM peak) and, beside them on
            # the side stream, the rare-tier kernel. The line's roofline is the
            # LONGER of the two, each timed alone by HIP events on its stream.
            d_ms, r_ms = fam_ms.get("dense", 0.0), fam_ms.get("rare", 0.0)
            wp = pairs_rank * width_words / (d_ms * 1e-3) if d_ms > 0 else 0.0
            tw = sparse_words["dense_words"] if sparse_words and sparse_words["sparse_words"] else width_words
            mfma = tw >= 64 and ctx.option("bitset_mfma") != 0
            if mfma:
                # the launched instantiation (bitset.hip bitset_mfma_kernel<KM, NS,
                # RAW, STORE, SPREAD>), so that traffic comes only from a PMC pass
                # taken on it; the default: raw 16-word stages, the next stage's DMA
                # spread between the MFMAs (round 6)
                def _o(name, dflt):
                    v = ctx.option(name)
                    return dflt if v is None else v
                if _o("bitset_mfma_raw", 1) and _o("bitset_mfma_km", 4) != 2 and not _o("bitset_mfma_store", 0):
                    sp_ = bool(_o("bitset_mfma_sched", 1))
                    pl_ = sp_ and bool(_o("bitset_mfma_plane", 1))
                    mfma_kinst = (f"bitset_mfma_kernel<4, 2, true, false, {'true' if sp_ else 'false'}, "
                                  f"{'true' if pl_ else 'false'}>")
                else:
                    mfma_kinst = "bitset_mfma_kernel"
                # the dense tiles on the matrix cores: pairs x W x 64 bit-products x 2 ops
                tops = pairs_rank * tw * 64 * 2 / (d_ms * 1e-3) / 1e12 if d_ms > 0 else 0.0
                dense_roof = {"bound": "mfma", "achieved": round(tops, 1), "peak": MFMA_FP4_PEAK_TOPS,
                              "unit": "TFLOP/s", "frac": round(tops / MFMA_FP4_PEAK_TOPS, 4),
                              "traffic": pmc_traffic(mfma_kinst),
                              "kernel": f"{mfma_kinst} (dense tier tiles, FP4 MFMA 32x32x64)",
                              "kernel_avg_ms": round(d_ms, 4), "ops_per_pair": 128 * tw,
                              "note": "algorithmic ops = pairs x W words x 64 bit-products x 2 (multiply + add) / "
                                      "the dense tile launch's own time (each kernel family timed alone: option serial_step); peak = the FP4 dense MFMA rate "
                                      "(MI355X_MICROARCH.md); the bits are e2m1 0.0 / 1.0 nibbles, sums exact in f32"}
            else:
                tops = wp * 4 / 1e12
                dense_roof = {"bound": "valu", "achieved": round(tops, 3), "peak": round(valu_peak, 3), "unit": "TOP/s",
                              "frac": round(tops / valu_peak, 4), "traffic": pmc_traffic("bitset_tile_kernel2"),
                              "kernel": "bitset_tile_kernel2 (dense tier tiles)", "kernel_avg_ms": round(d_ms, 4),
                              "ops_per_pair": 4 * width_words,
                              "note": "lane-ops of the dense tier (pairs x W word pairs x 4) / the dense tile launches' "
                                      "own time; peak = measured and+bcnt issue ceiling "
                                      "(profiles/r01/valu_microbench.txt)",
                              "hbm_streaming_model": {"achieved": round(algo_bytes / (d_ms * 1e-3) / 1e9, 1) if d_ms else 0,
                                                      "bytes_per_pair": bytes_per_pair,
                                                      "note": "16*W B/pair (SURVEY 8d), operands reused from LDS"}}
            roof = dense_roof
            v_ms = fam_ms.get("variant", 0.0)
            cands = [(d_ms, dense_roof)]
            if v_ms > 0 and variant:
                f_pairs = pairs_rank / max(1, N * (N - 1) // 2)
                f_rows = (r1 - r0) / N
                mb = variant.get("member_bytes", 12) if ctx.option("variant_short") != 0 else 12
                if mb == 4:
                    # grouped rare tier (C3): the short-list walk reads one packed
                    # member (4 B: set | mask << 16) per product and per row entry
                    # its set-side record (8 B) and its own packed mask (4 B)
                    v_bytes = 4.0 * variant["products"] * f_pairs + 12.0 * variant["entries"] * f_rows
                    vk = "variant_short_kernel"
                    vnote = ("algorithmic bytes = 4 B per product (the packed list member) + 12 B per row entry "
                             "(set-side record + its own mask); products = the block's share of the tier's sum "
                             "over words of z(z-1)/2")
                else:
                    # variant tier (C4): each product reads one list member (8 B packed
                    # set << 47 | mask, or 4 B set + 8 B mask, coalesced along the
                    # word's list) for a row entry (its record: 4 B entry + 8 B mask
                    # + 8 B list bounds)
                    v_bytes = float(mb) * variant["products"] * f_pairs + 20.0 * variant["entries"] * f_rows
                    vk = "variant_rows_kernel"
                    vnote = (f"algorithmic bytes = {mb} B per product (the list member's set and mask) "
                             "+ 20 B per row entry; products = the block's share of the tier's "
                             "sum over words of z(z-1)/2")
                ach = v_bytes / (v_ms * 1e-3) / 1e9
                cands.append((v_ms, {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                                     "frac": round(ach / HBM_PEAK_GBS, 4),
                                     "traffic": pmc_traffic(vk),
                                     "kernel": f"{vk} (variant tier; in the step beside the dense tiles, timed alone)",
                                     "kernel_avg_ms": round(v_ms, 4), "algo_bytes_per_launch": round(v_bytes),
                                     "note": vnote}))
            if r_ms > 0 and rare:
                # rare tier, row-major walk (rare_rows_kernel) or list-major
                # (rare_pairs_kernel): its useful bytes = the rows' (set, list)
                # records (8 B list + 4 B weight + 2 B skip) + one 4-byte member
                # read per pair increment + the I updates (4 B read + 4 B write
                # per pair of the block)
                rec, incs = sets.rare_info()[2], sets.rare_stats()[0]
                f_rows = (r1 - r0) / N
                f_pairs = pairs_rank / max(1, N * (N - 1) // 2)
                # list members: 2 bytes for collections of <= 65,536 sets (option rare_u16)
                mbytes = 2.0 if N <= 65536 and ctx.option("rare_u16") != 0 else 4.0
                rare_bytes = 14.0 * rec * f_rows + mbytes * incs * f_pairs + 8.0 * pairs_rank
                # row-major: past one 16,384-column LDS chunk the direct walk
                # (every record once, atomics into I; option rare_direct)
                rk = "rare_pairs_kernel"
                if sets.block_cost((r0, r1))[1] == 1:
                    rk = "rare_rows_direct_kernel" if N > 16384 and ctx.option("rare_direct") != 0 else "rare_rows_kernel"
                ach = rare_bytes / (r_ms * 1e-3) / 1e9
                rare_roof = {"bound": "hbm", "achieved": round(ach, 1), "peak": HBM_PEAK_GBS, "unit": "GB/s",
                             "frac": round(ach / HBM_PEAK_GBS, 4), "traffic": pmc_traffic(rk.rsplit("_kernel", 1)[0]),
                             "kernel": f"{rk} (rare tier; in the step beside the dense tiles, timed alone)", "kernel_avg_ms": round(r_ms, 4),
                             "algo_bytes_per_launch": round(rare_bytes),
                             "member_bytes": mbytes,
                             "note": "algorithmic bytes = 14 B per (set, list) record of the rows + one list member "
                                     "read per pair increment (member_bytes) + 8 B per pair of I updated"}
                cands.append((r_ms, rare_roof))
            # the line's roofline is the longest kernel family's; the others ride along
            cands.sort(key=lambda c: -c[0])
            roof = dict(cands[0][1])
            if len(cands) > 1:
                roof["other"] = [c[1] for c in cands[1:]]
            roof["step_kernel_span_ms"] = round(k_avg_ms, 4)
        else:
            kname = {"sorted": "sorted_join_kernel",
                     "sketch": ("sketch_tile_kernel<16,24,LDS,K=2>" if sk_whole else
                                "sketch_ring_kernel (32x32, interleaved LDS rings, step-synchronised phases)")}[method]
            kms = fam_ms.get("sorted", k_avg_ms) if method == "sorted" else k_avg_ms
            achieved = algo_bytes / (kms * 1e-3) / 1e9 if kms > 0 else 0.0
            peak = LDS_B32_PEAK_GBS if method == "sketch" else HBM_PEAK_GBS
            roof = {"bound": "lds" if method == "sketch" else "hbm", "achieved": round(achieved, 1), "peak": peak,
                    "unit": "GB/s", "frac": round(achieved / peak, 4), "traffic": pmc_traffic(kname.split(" ")[0]),
                    "kernel": kname, "kernel_avg_ms": round(kms, 4), "step_kernel_span_ms": round(k_avg_ms, 4),
                    "algo_bytes_per_launch": algo_bytes, "bytes_per_pair": bytes_per_pair}
        def with_readings(rf):
            """A roofline (and its `other` families) with the PMC readings of
            ITS kernel: each pmc_traffic(kern) lookup filed its own."""
            if not isinstance(rf, dict):
                return rf
            name = rf.get("kernel", "").split(" (")[0].replace(" ", "")
            rd = next((v for k, v in traffic_readings.items()
                       if name == k.replace(" ", "") or ("<" not in k and name.startswith(k))), None)
            out_rf = dict(rf, traffic_readings=rd)
            if isinstance(rf.get("other"), list):
                out_rf["other"] = [with_readings(o) for o in rf["other"]]
            return out_rf

        # ---------------------------------------------------------------- CPU baseline
        cpu = None
        cpu_opt = None
        host = host_cpus()
        if not args.no_cpu_baseline and world == 1:
            cpu, cpu_opt = cpu_baselines(cfg, args.cpu_threads or host["threads"], host)
        out = {
            "metric": "genome-pair distances/sec (N×N)",
            "value": round(value, 1),
            "unit": "pairs/s",
            "end_to_end_pairs_per_s": round(pairs_job / e2e_s, 1),
            "n_gpus": world,
            "steps": args.steps,
            "warmup": args.warmup,
            "ms_per_step": round(elapsed_max / args.steps * 1e3, 4),
            "higher_is_better": True,
            "scaling": "weak",
            "vs_baseline": None,
            "dtype": "u64" if method != "sketch" else "i32",
            "data": "synthetic (splitmix64 genomes, SURVEY 8d)",
            "config": config,
            "roofline": with_readings(roof),
            "verified": verified,
            "cpu_baseline": cpu,
            "cpu_optimized": cpu_opt,
            "setup_s": setup,
            "end_to_end": {"pairs_per_s": round(pairs_job / e2e_s, 1), "seconds": round(e2e_s, 3),
                           "first_call_s": round(first_call_s, 4) if first_call_s is not None else None,
                           "plan_s": (round(first_call_s - elapsed_max / args.steps, 4)
                                      if first_call_s is not None else None),
                           "host_buffer": "pageable" if args.pageable else "page-locked (gdist_host_alloc)",
                           "note": "one pass over the collection from FASTA bytes in host memory: pack (H2D + "
                                   "kmer extraction + sort) + represent (dictionary, bitsets, sparse words) + the "
                                   "FIRST matrix call (it builds the region's launch plans, geometry only, then "
                                   "runs; plan_s = that call minus a steady step); synthetic-genome "
                                   "generation and the release of the caller's host buffer (setup_s.host_free) "
                                   "excluded; max over ranks"},
            "dumped": dumped,
            "full": True,
        }
        print(json.dumps(out), flush=True)
    if verified is not None and not verified["ok"]:
        log(f"rank {rank}: device output disagrees with the independent recount")
        sys.exit(1)
    teardown()


DUMP_BYTES = 64 << 20                # --dump-outputs writes at most this much, all ranks together
DUMP_SEED = 0


def dump_outputs(outdir, dI, dD, N, r0, r1, rank=0, world=1):
    """Write this rank's block of the step's outputs, read back from the
    device buffers the timed steps wrote: I (|A∩B|, or the sketches' common
    count) and D (the fp64 distance), both as float64 (the counts are exact
    in it), to outdir/I.npy and outdir/D.npy (I_rank<r>.npy, D_rank<r>.npy
    when there are several ranks). The step computes the upper triangle and
    leaves entries with column <= row untouched (include/gdist.h), so they
    are written as 0. A block past the byte limit is cut to a fixed sample
    of its rows (and, past one row, of its columns) drawn from DUMP_SEED:
    the same arguments give the same sample."""
    rows = r1 - r0
    budget = DUMP_BYTES // world // 16            # elements of each array: 8 B in I + 8 B in D
    ncol = min(N, max(1, budget))
    nrow = min(rows, max(1, budget // ncol))
    rng = np.random.default_rng(DUMP_SEED)
    pick_r = np.arange(rows) if nrow == rows else np.sort(rng.choice(rows, nrow, replace=False))
    pick_c = np.arange(N) if ncol == N else np.sort(rng.choice(N, ncol, replace=False))
    if nrow == rows and rows > 0:
        I = dI.to_host(np.int32, rows * N).reshape(rows, N)
        D = dD.to_host(np.float64, rows * N).reshape(rows, N)
    else:
        I = np.zeros((nrow, N), np.int32)
        D = np.zeros((nrow, N), np.float64)
        for t, r in enumerate(pick_r):
            I[t] = dI.to_host(np.int32, N, int(r) * N)
            D[t] = dD.to_host(np.float64, N, int(r) * N)
    untouched = np.arange(N)[None, :] <= (r0 + pick_r)[:, None]
    I = np.where(untouched, 0, I)[:, pick_c].astype(np.float64)
    D = np.where(untouched, 0.0, D)[:, pick_c]
    os.makedirs(outdir, exist_ok=True)
    suffix = f"_rank{rank}" if world > 1 else ""
    names = []
    for name, a in (("I", I), ("D", D)):
        np.save(os.path.join(outdir, f"{name}{suffix}.npy"), np.ascontiguousarray(a))
        names.append(f"{name}{suffix}.npy")
    return {"dir": outdir, "arrays": names, "dtype": "float64", "rows": int(nrow), "of_rows": int(rows),
            "cols": int(ncol), "of_cols": int(N), "seed": DUMP_SEED,
            "what": "the last timed step's I and D of this rank's rows; entries with column <= row hold 0"}


def _kmer_codes(seq: bytes, k: int, protein: bool) -> np.ndarray:
    """Independent numpy recount of one synthetic genome's kmer codes (DESIGN.md
    §3 packing spec; synthetic genomes hold only ACGT / the 20 standard
    residues, upper case): protein k<=8 = raw bytes big-endian; DNA = 2-bit
    A0 C1 G2 T3, first base most significant, both strands (union)."""
    a = np.frombuffer(seq, np.uint8)
    if len(a) < k:
        return np.zeros(0, np.uint64)
    if protein:
        assert k <= 8
        sym = a.astype(np.uint64)
        bits = 8
    else:
        lut = np.full(256, 255, np.uint8)
        for i, c in enumerate(b"ACGT"):
            lut[c] = i
        sym = lut[a]
        assert sym.max() < 4
        sym = sym.astype(np.uint64)
        bits = 2

    def windows(x):
        w = np.lib.stride_tricks.sliding_window_view(x, k)
        c = np.zeros(len(w), np.uint64)
        for t in range(k):
            c = (c << np.uint64(bits)) | w[:, t]
        return c

    if protein:
        return np.unique(windows(sym))
    rc = (np.uint64(3) - sym)[::-1].copy()
    return np.unique(np.concatenate([windows(sym), windows(rc)]))


def verify_sample(cfg, method, N, r0, r1, dI, dD, max_over_ranks, npairs=4, step=None):
    """Recount |A∩B| and the distance of a few pairs of this rank's row block
    from regenerated genomes and compare them bit-exactly with the device
    output of a step; every rank checks its own rows (so the multi-GPU
    exchange is covered) and the verdict is the MIN over ranks. The sampled
    pairs' outputs are poisoned (I = -7, D = 42.5) and one more step (the
    timed loop's replayed graph) runs before they are read back (VERDICT r5
    item 1): a replay that skipped a kernel family would show."""
    if method == "sketch":
        return None
    from gdist import synth
    rows = [i for i in sorted({r0, (r0 + r1) // 2, r1 - 1}) if r0 <= i < r1 and i < N - 1]
    cand = []
    for i in rows:
        for j in (i + 1, N - 1, (i + N) // 2):
            if i < j < N and (i, j) not in cand:
                cand.append((i, j))
    cand = cand[:npairs]
    ok, cache = 1.0, {}
    if step is not None:
        for (i, j) in cand:
            o = (i - r0) * N + j
            dI.from_host(np.array([-7], np.int32), o)
            dD.from_host(np.array([42.5]), o)
        step()

    def codes(g):
        if g not in cache:
            if cfg.get("realistic"):
                s = synth.realistic_genome(g, cfg["length"], cfg["p_max"], cfg["cfg"], protein=cfg["protein"])
            else:
                s = bytes(synth.genomes(1, cfg["length"], cfg["p_max"], cfg["cfg"], protein=cfg["protein"],
                                        first=g)[0])
            cache[g] = _kmer_codes(s, cfg["k"], cfg["protein"])
        return cache[g]

    for (i, j) in cand:
        a, b = codes(i), codes(j)
        inter = len(np.intersect1d(a, b, assume_unique=True))
        union = len(a) + len(b) - inter
        d = 1.0 - inter / union if inter > 0 else 1.0
        o = (i - r0) * N + j
        gi = int(dI.to_host(np.int32, 1, o)[0])
        gd = dD.to_host(np.float64, 1, o)
        if gi != inter or gd.view(np.uint64)[0] != np.array([d]).view(np.uint64)[0]:
            log(f"verify: pair ({i},{j}) device I={gi} D={gd[0]!r}, recount I={inter} D={d!r}")
            ok = 0.0
    ok = max_over_ranks(-ok) * -1.0          # MIN over ranks
    return {"pairs_per_rank": len(cand), "ok": bool(ok == 1.0), "poisoned": step is not None,
            "how": "independent numpy recount from regenerated genomes, bit-exact I and fp64 D, "
                   "read after a replayed step into outputs poisoned at the sampled pairs"}


def host_cpus() -> dict:
    """The CPUs this process may use and what they are. On the GPU box
    os.cpu_count() reports the whole machine while the job's share is set by
    its affinity mask and OMP_NUM_THREADS (16 per GPU there), so the CPU legs
    run on min(affinity, OMP_NUM_THREADS) threads and all three are recorded."""
    model = ""
    try:
        with open("/proc/cpuinfo") as f:
            for line in f:
                if line.startswith("model name"):
                    model = line.split(":", 1)[1].strip()
                    break
    except OSError:
        pass
    try:
        aff = len(os.sched_getaffinity(0))
    except (AttributeError, OSError):
        aff = os.cpu_count() or 1
    omp = os.environ.get("OMP_NUM_THREADS", "")
    threads = min(aff, int(omp)) if omp.isdigit() and int(omp) > 0 else aff
    return {"model": model, "os_cpu_count": os.cpu_count(), "affinity": aff, "omp_num_threads": omp or None,
            "threads": threads}


def cpu_baselines(cfg, threads, host=None, target_s=10.0, cap=6000, batch=20):
    """The Java-faithful restatement (HashSet<String> + FastaDistanceProcessor
    loop, the reference's default batch of 20 cached rows,
    FastaDistanceProcessor.java:88) on a bounded sample — the rows of the
    first batch against the later genomes of a prefix of the workload — plus
    the optimised sorted-merge CPU path on rows 0..T-1. Each prefix is
    calibrated so the leg runs ~target_s seconds."""
    sys.path.insert(0, os.path.join(ROOT, "oracle"))
    import oracle
    from gdist import synth
    T = max(1, threads)
    kind = 1 if cfg["protein"] else 0
    cap = max(T + 2, min(cap, int(2e8 // cfg["length"])))    # bound the sample's residues too

    def genomes(n):
        if cfg.get("realistic"):
            return synth.realistic_genomes(n, cfg["length"], cfg["p_max"], cfg["cfg"], protein=cfg["protein"])
        return [bytes(r) for r in synth.genomes(n, cfg["length"], cfg["p_max"], cfg["cfg"], protein=cfg["protein"])]

    def faithful(n):
        seqs = genomes(n)
        t = time.perf_counter()
        pairs, _ = oracle.faithful_fasta_dist(seqs, cfg["k"], kind, 0, batch=batch, max_rows=batch, nthreads=T)
        return pairs, time.perf_counter() - t

    def optimised(n):
        off, codes = oracle.pack(genomes(n), cfg["k"], kind, 0)
        t = time.perf_counter()
        oracle.matrix(off, codes, 0, T, 0, n, flags=0x100, nthreads=T)
        return T * n - T * (T + 1) // 2, time.perf_counter() - t

    def calibrated(run, n0):
        n = n0
        pairs, dt = run(n)
        for _ in range(4):          # fixed costs make small runs look slow: grow in steps
            if dt >= target_s / 2 or n >= cap:
                break
            n = min(cap, max(n + 1, int(n * min(50.0, target_s / max(dt, 1e-3)))))
            pairs, dt = run(n)
        return n, pairs, dt

    n1, p1, dt1 = calibrated(faithful, batch + max(1, batch // 2))
    fa = {"value": round(p1 / dt1, 3), "unit": "pairs/s", "cores": T, "kind": "port", "host": host,
          "sample": f"rows 0..{batch - 1} x all later columns of the first {n1} genomes ({p1} pairs, "
                    f"batch {batch} as FastaDistanceProcessor.java:88: cached rows + per-pair rebuilt sets as "
                    f":150-186, rows in parallel on {T} threads as :157-158), {dt1:.1f} s"}
    n2, p2, dt2 = calibrated(optimised, T + max(1, T // 2))
    opt = {"value": round(p2 / dt2, 2), "unit": "pairs/s", "cores": T, "kind": "port-optimised",
           "sample": f"rows 0..{T - 1} x all later columns of the first {n2} genomes ({p2} pairs), "
                     f"sorted-uint64 merge, OpenMP, {dt2:.1f} s"}
    return fa, opt


if __name__ == "__main__":
    main()
