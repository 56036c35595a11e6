"""Which test runs each tuning option's non-default values against the oracle.

One entry per name of GDIST_OPTIONS (csrc/gdist_internal.hpp), of exactly one
kind:

  covered_by  [(file, function, values)]: that test sets the option to each of
              `values` and compares counts and distances with the oracle
  sweep       the non-default values tests/test_gpu_option_sweep.py runs, in
              the rows of SCENE_K / SCENE_S / SCENE_T below
  exempt      why the option cannot reach a result

tests/test_option_table.py (no GPU) keeps the keys equal to GDIST_OPTIONS,
checks that every covered_by target exists and names its option, and that
every sweep value is a parameter id of the sweep file. A plain module: no
conftest, no fixtures.
"""

PARITY = "tests/test_gpu_parity.py"
VARIANT = "tests/test_gpu_variant.py"
BATCHES = "tests/test_gpu_sparse_batches.py"
BALANCE = "tests/test_gpu_sparse_balance.py"
REALISTIC = "tests/test_gpu_realistic.py"
CLOSEST = "tests/test_gpu_closest.py"
MR = "tests/mr_worker.py"
RCCL = "tests/rccl_worker.py"

SPARSE_SWEEP = "test_sparse_complement_words_exact"      # its settings: SPARSE_MODES
MFMA = "test_dense_tiles_mfma_exact"
RARE = "test_rare_tier_thresholds_exact"
SKETCH = "test_sketch_merge_edges_vs_oracle"
VTIER = "test_variant_tier_exact"


def covered(*targets):
    return {"covered_by": list(targets)}


def sweep(*values):
    return {"sweep": list(values)}


OPTIONS = {
    "trace": {"exempt": "prints stage times and plans to stderr after a stream synchronise (Trace, gdist_ctx::trace): "
                        "it picks no kernel, tiling or threshold"},
    "rare_t": covered((PARITY, SPARSE_SWEEP, [2]), (VARIANT, VTIER, [3])),
    "rare_dedup": covered((PARITY, RARE, [0])),
    "rare_kernel": covered((PARITY, RARE, [0, 1])),
    "rare_overlap": sweep(0),
    "bitset_diag": sweep(0),
    "bitset_partial_rr": sweep(7, 0),
    "bitset_wg_per_cu": sweep(64, 1, 3),
    "bitset_min_chunks": sweep(1, 1000, 5),
    "reps_block": covered((PARITY, "test_greedy_reps_device", [100, 37]), (MR, "run_case", [100])),
    "locus_order": covered((PARITY, SPARSE_SWEEP, [0])),
    "sparse": covered((PARITY, SPARSE_SWEEP, [0])),
    "sparse_zmax": covered((PARITY, SPARSE_SWEEP, [100000, 40, 12])),
    "sparse_wg_per_cu": sweep(1, 16),
    "sparse_sun": covered((PARITY, SPARSE_SWEEP, [2, 3, 4])),
    "sparse_dyn": covered((PARITY, SPARSE_SWEEP, [0])),
    "sparse_batch": covered((BATCHES, "test_batches_exact", [48, 5, 1])),
    "sparse_wtail": covered((BATCHES, "test_batches_exact", [0])),
    "sparse_diag22": covered((PARITY, SPARSE_SWEEP, [0])),
    "sparse_rpart22": covered((PARITY, SPARSE_SWEEP, [0])),
    "sparse_mt": covered((PARITY, SPARSE_SWEEP, [1])),
    "sketch_k": sweep(1, 4, 6),
    "sketch_tile": sweep(16),
    "sketch_v2": covered((PARITY, SKETCH, [0])),
    "sketch_phase": sweep(0),
    "sketch_cap": covered((PARITY, SKETCH, [2, 7, 8, 15, 64, 120, 255, 300, 5000])),
    "sketch_ring": covered((PARITY, SKETCH, [16, 32, 128, 512])),
    "sketch_wait": covered((PARITY, SKETCH, [1])),
    "sparse_part_budget": covered((PARITY, SPARSE_SWEEP, [0])),
    "guides": covered((PARITY, SPARSE_SWEEP, [4]), (VARIANT, "test_grouped_rare_tier_keyless", [0])),
    "force_exchange": covered((RCCL, "main", [1])),
    "sparse_chunks": covered((PARITY, SPARSE_SWEEP, [3, 5, 6, 7, 13, 37]), (BALANCE, "test_balanced_chunks_exact", [1, 2])),
    "graph": sweep(0),
    "time_kernels": sweep(1),
    "step_timing": sweep(1),
    "sparse_rare": covered((PARITY, SPARSE_SWEEP, [0])),
    "sparse_fused": covered((PARITY, SPARSE_SWEEP, [0])),
    "sparse_fold": covered((PARITY, SPARSE_SWEEP, [0, 100000])),
    "fill_sort": covered((PARITY, "test_bitset_fill_ragged_sets", [0, 1, 2, 5]), (PARITY, SPARSE_SWEEP, [4]),
                         (VARIANT, VTIER, [3])),
    "pack_sort": covered((PARITY, SPARSE_SWEEP, [1])),
    "pack_summary": covered((PARITY, SPARSE_SWEEP, [0])),
    "pack_code_sort": covered((PARITY, "test_pack_random_modes", [0])),
    "pack_overlap": covered((PARITY, "test_chunked_pack_bitset_matrix", [0, 2])),
    "pack_chunk": covered((PARITY, "test_chunked_pack_bitset_matrix", [40000])),
    "exchange_budget": covered((MR, "run_case", [1 << 30])),
    "pack_codes_budget": covered((PARITY, "test_chunked_pack_bitset_matrix", [0])),
    "sparse_groups": covered((REALISTIC, "test_realistic_group_tier_exact", [0])),
    "sparse_xcd": covered((PARITY, SPARSE_SWEEP, [1])),
    "rare_u16": covered((PARITY, RARE, [0])),
    "rare_rows_threads": covered((PARITY, RARE, [256, 1024])),
    "rare_direct": covered((PARITY, RARE, [1]), (VARIANT, "test_variant_walk_across_column_chunks", [0])),
    "bitset_mfma": covered((PARITY, MFMA, [0])),
    "bitset_mfma_raw": covered((PARITY, MFMA, [0])),
    "bitset_mfma_km": covered((PARITY, MFMA, [2])),
    "bitset_mfma_ns": covered((PARITY, MFMA, [3, 4])),
    "bitset_mfma_splits": covered((PARITY, MFMA, [3]), (PARITY, "test_dense_tiles_mfma_past_f32_bound", [1])),
    "bitset_mfma_group": covered((PARITY, MFMA, [2])),
    "bitset_mfma_store": covered((PARITY, MFMA, [1])),
    "bitset_mfma_sched": covered((PARITY, MFMA, [0])),
    "sketch_perm": covered((PARITY, SKETCH, [0])),
    "bitset_mfma_plane": covered((PARITY, MFMA, [0])),
    "sort_radix": covered((PARITY, SPARSE_SWEEP, [10])),
    "variant": covered((VARIANT, VTIER, [1, 0])),
    "variant_dmin": covered((VARIANT, VTIER, [120]), (VARIANT, "test_variant_greedy_reps", [30])),
    "range_summary": sweep(0, 1),
    "rare_c16": covered((PARITY, "test_rare_rows_heavy_rows_exact", [0]), (PARITY, RARE, [0])),
    "variant_c16": covered((VARIANT, "test_variant_walk_across_column_chunks", [0])),
    "variant_split": covered((VARIANT, "test_variant_walk_across_column_chunks", [1, 3])),
    "rare_group": covered((VARIANT, "test_grouped_rare_tier_keyless", [1, 2]), (REALISTIC, "test_realistic_twins_exact", [0])),
    "variant_short": covered((VARIANT, VTIER, [0])),
    "epilogue_rows": covered((PARITY, "test_distance_epilogue_modes", [0])),
    "variant_pack_keyless": covered((VARIANT, "test_grouped_rare_tier_exact", [0])),
    "variant_key2": covered((VARIANT, VTIER, [0])),
    "variant_keyless_rare": covered((VARIANT, VTIER, [1])),
    "variant_bits": covered((VARIANT, VTIER, [64])),
    "dense_first": sweep(0, 1),
    "reps_split": covered((MR, "run_case", [0])),
    "serial_step": sweep(1),
    "split_build": covered((VARIANT, "test_split_build_equals_whole_build", [3]), (MR, "run_case", [0])),
    "closest_rows": covered((CLOSEST, "test_chunking", [1, 7, 64, 128])),
    "closest_cols": covered((CLOSEST, "test_chunking", [33, 64, 100, 193])),
    "sparse_balance": covered((BALANCE, "test_balanced_chunks_exact", [0, 1])),
}

# ---------------------------------------------------------------------------
# Rows of tests/test_gpu_option_sweep.py::test_option_values_exact:
# (base, options, kind). `base` names the collection and the options it is
# built with (BASES there); `kind` the reach the case asserts.
SCENE_K = [
    # diagonal tiles through the ordinary tile launch: beside the MFMA tiles'
    # plan (640 dense words), by AND + popcount, and beside the sparse tiles
    ("dense", dict(bitset_diag=0), "diag"),
    ("dense", dict(bitset_diag=0, bitset_mfma=0), "diag"),
    ("mixed", dict(bitset_diag=0), "diag"),
    ("mixed", dict(bitset_diag=0, bitset_mfma=0), "diag"),
    # the AND + popcount tiles' K split over 82 chunks: a chunk a workgroup,
    # 5 splits (the last of 17 chunks' worth holds 14), one split, 16 splits
    # of 6 chunks (the 14th holds 4, the last two none)
    ("dense82", dict(bitset_mfma=0, bitset_wg_per_cu=64, bitset_min_chunks=1), "ksplit_chunk"),
    ("dense82", dict(bitset_mfma=0, bitset_wg_per_cu=1, bitset_min_chunks=16), "ksplit_ragged"),
    ("dense82", dict(bitset_mfma=0, bitset_wg_per_cu=16, bitset_min_chunks=1000), "ksplit_one"),
    ("dense82", dict(bitset_mfma=0, bitset_wg_per_cu=3, bitset_min_chunks=5), "ksplit_ragged"),
    # the last row tile of 44 rows (RR = 3) in the whole-tile launches
    # (bitset_partial_rr 0), and 7 as the largest RR with launches of its own
    ("dense", dict(bitset_mfma=0, bitset_partial_rr=0), "partial"),
    ("dense", dict(bitset_mfma=0, bitset_partial_rr=7), "partial"),
    # the rare kernels in line on the main stream
    ("dense", dict(rare_overlap=0, rare_kernel=0), "rare_inline"),
    ("dense", dict(rare_overlap=0, rare_kernel=1), "rare_inline"),
    ("split_rare", dict(rare_overlap=0, rare_kernel=0), "rare_inline"),
    ("split_rare", dict(rare_overlap=0, rare_kernel=1), "rare_inline"),
    # the side stream's families on the main stream ahead of the dense tiles
    ("mixed", dict(serial_step=1), "serial"),
    ("mixed", dict(serial_step=1, dense_first=1), "serial"),
    ("variant", dict(serial_step=1), "serial"),
    ("variant", dict(serial_step=1, dense_first=1), "serial"),
    # the dense tiles issued after the side stream's launches where they go
    # first by default (no sparse words), and first where they go last
    ("variant", dict(dense_first=0), "order"),
    ("mixed", dict(dense_first=1), "order"),
    # (exactness only: ~626 sparse words bind the chunk count whatever the
    # target; SCENE_T's test_sparse_wg_per_cu_chunk_counts shows the counts)
    ("split", dict(sparse_wg_per_cu=1), "sparse_plan"),
    ("split", dict(sparse_wg_per_cu=16), "sparse_plan"),
    ("split", dict(graph=0), "no_graph"),
    # the one-sort summary asked for in a build split into three shares of
    # code ranges, and the code-range summary at a size that would not take it
    ("split", dict(range_summary=0, split_build=3), "split_build"),
    ("split", dict(range_summary=1), "summary"),
]

# Rows of test_sketch_tile_paths_exact: (options, [(width, launch path)]).
# 40 sketches of a 16 x 24 tile fit LDS up to a row stride of 1,020 dwords, 32
# of a 16 x 16 tile up to 1,275 (sketch.hip: LDS_SK_MAX, sketch_stride; the
# test derives the paths from those and compares): width 1100 is the 16 x 16
# LDS tile without the option, 1273 the widest every variant keeps in LDS,
# 1275 the V2 rows' (two sentinels wider) first global-memory width and the
# plain rows' last in LDS, 1500 global memory for all.
_MERGES = [dict(), dict(sketch_v2=0), dict(sketch_v2=0, sketch_k=4), dict(sketch_v2=0, sketch_k=1),
           dict(sketch_v2=0, sketch_k=6)]
SCENE_S = []
for _m in _MERGES:
    _v2 = not _m
    SCENE_S.append((dict(sketch_phase=0, sketch_tile=16, **_m), [(64, "lds16x16"), (1000, "lds16x16")]))
    SCENE_S.append((dict(sketch_phase=0, **_m), [(1100, "lds16x16"), (1273, "lds16x16"),
                                                 (1275, "global" if _v2 else "lds16x16"), (1500, "global")]))

# The sweep file's tests outside the scene K and S rows, each parametrised by its option
SCENE_T = {
    # on a collection of ~12,400 sparse words and 55 tiles, where the chunk
    # count follows the target (the scene K rows above cannot show it)
    "test_sparse_wg_per_cu_chunk_counts": [dict(sparse_wg_per_cu=1), dict(sparse_wg_per_cu=16)],
    "test_step_timing_of_replayed_steps": [dict(step_timing=1)],
    "test_time_kernels_matrix_families": [dict(time_kernels=1)],
}
