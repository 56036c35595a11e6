"""Host-side mirrors of the hot-path processors, driving libgdist.so.

Each function keeps the reference processor's options, defaults, validation
errors and output format, and replaces its per-pair Java loop with whole
row-block / row-query calls on the device:

  fasta_distance   FastaDistanceProcessor  (fastaDist)  FastaDistanceProcessor.java:84-194
  fasta_close_pairs  the fastaDist lines with distance <= max_dist (KmerSets.within)
  genome_distance  GenomeProcessor         (genomes)    GenomeProcessor.java:74-150
  genomes_against  the same table over a resident base collection (KmerSets.cross_*)
  fasta_reps       FastaDistanceRepsProcessor (fastaReps) FastaDistanceRepsProcessor.java:58-149
  distance_reps    DistanceRepsProcessor   (distReps)   DistanceRepsProcessor.java:140-275
  width_processor  WidthProcessor          (width)      WidthProcessor.java:88-208
  distance_check   DistanceCheckProcessor  (distCheck)  DistanceCheckProcessor.java:149-223

Output rows are emitted in (row, column) order; the reference's fastaDist
order is nondeterministic (rows run in parallel, FastaDistanceProcessor.java:157,188),
so consumers compare those outputs as sets of lines.
"""
from __future__ import annotations

import dataclasses
from typing import Iterable, Iterator, Sequence, TextIO

import numpy as np

from . import _lib as L
from .fasta import Sequence as FastaRecord
from .javafmt import java_double, java_format_f
from .kmers import Context, KmerSets, KmerType, SketchSets


class ParseFailureException(ValueError):
    """org.theseed.basic.ParseFailureException (bad command parameters)."""


@dataclasses.dataclass
class Genome:
    """The part of org.theseed.genome.Genome the distance path reads: contig
    DNA (GenomeKmers), protein sequences (ProteinKmers, the `prot` method)
    and the taxonomic lineage rank -> taxon (TaxonDistanceMethod)."""
    id: str
    name: str
    contigs: list[str]
    proteins: list[str] = dataclasses.field(default_factory=list)
    lineage: dict = dataclasses.field(default_factory=dict)

    def kmer_text(self) -> bytes:
        # contigs joined by the 0x00 separator: one set, no kmer spans contigs
        return b"\0".join(c.encode("latin-1") for c in self.contigs)


def _row_blocks(n: int, block: int) -> Iterator[tuple[int, int]]:
    for r0 in range(0, n, block):
        yield r0, min(n, r0 + block)


def fasta_distance(records: Sequence[FastaRecord], out: TextIO, kmer_size: int = 0, batch: int = 20,
                   kmer_type: KmerType = KmerType.DNA, flags: int = 0, method: int = L.METHOD_AUTO,
                   ctx: Context | None = None, row_block: int = 1024) -> int:
    """fastaDist: N×N upper triangle of kmer distances over FASTA records."""
    k = kmer_size or kmer_type.getKmerSize()                       # FastaDistanceProcessor.java:95-96
    if k < 2:
        raise ParseFailureException("Kmer size must be at least 2.")   # FastaDistanceProcessor.java:98-99
    if batch < 1:
        raise ParseFailureException("Batch size must be at least 1.")  # FastaDistanceProcessor.java:101-102
    out.write("seq1\tname1\tseq2\tname2\tdistance\n")                 # FastaDistanceProcessor.java:139
    n = len(records)
    if n < 2:
        return 0
    sets = KmerSets.from_sequences([r.sequence for r in records], k, kmer_type, flags, ctx)
    if method == L.METHOD_BITSET:
        sets.build_bitsets()
    pairs = 0
    for r0, r1 in _row_blocks(n, row_block):
        _, D = sets.matrix((r0, r1), (0, n), upper=True, method=method, want_I=False)
        for a in range(r0, r1):
            ra = records[a]
            row = D[a - r0]
            for j in range(a + 1, n):
                rb = records[j]
                out.write(f"{ra.label}\t{ra.comment}\t{rb.label}\t{rb.comment}\t{java_double(row[j])}\n")
                pairs += 1
    return pairs


def fasta_close_pairs(records: Sequence[FastaRecord], out: TextIO, max_dist: float, kmer_size: int = 0,
                      kmer_type: KmerType = KmerType.DNA, flags: int = 0, method: int = L.METHOD_AUTO,
                      ctx: Context | None = None) -> int:
    """fastaDist restricted to the close pairs: the header, then exactly those
    lines of fasta_distance whose distance is <= max_dist, in the same order,
    from one KmerSets.within(upper=True) call; the N×N stays on the device.
    Returns the lines written."""
    k = kmer_size or kmer_type.getKmerSize()
    if k < 2:
        raise ParseFailureException("Kmer size must be at least 2.")
    out.write("seq1\tname1\tseq2\tname2\tdistance\n")
    n = len(records)
    if n < 2:
        return 0
    sets = KmerSets.from_sequences([r.sequence for r in records], k, kmer_type, flags, ctx)
    if method == L.METHOD_BITSET:
        sets.build_bitsets()
    rowptr, cols, d = sets.within(max_dist, upper=True, method=method)
    for a in range(n):
        ra = records[a]
        for p in range(rowptr[a], rowptr[a + 1]):
            rb = records[cols[p]]
            out.write(f"{ra.label}\t{ra.comment}\t{rb.label}\t{rb.comment}\t{java_double(d[p])}\n")
    return int(rowptr[n])


def genome_distance(base: Sequence[Genome], others: Sequence[Sequence[Genome]], out: TextIO,
                    kmer_size: int = 21, max_dist: float = 0.9, flags: int = 0,
                    method: int = L.METHOD_AUTO, ctx: Context | None = None, within: bool = False) -> int:
    """genomes: every comparison genome against every base genome. The
    reference validates max_dist and then writes every pair
    (GenomeProcessor.java:140-144); within=True applies the filter its usage
    text documents (GenomeProcessor.java:35): only the pairs with distance <=
    max_dist are written, from one KmerSets.within call."""
    if kmer_size < 4:
        raise ParseFailureException("Kmer size cannot be less than 4.")          # GenomeProcessor.java:84-85
    if max_dist <= 0.0 or max_dist > 1.0:
        raise ParseFailureException("Maximum distance must be > 0 and <= 1.")    # GenomeProcessor.java:89-90
    out.write("genome1\tgenome2\tdistance\n")                                    # GenomeProcessor.java:121
    comps = [g for src in others for g in src]
    if not base or not comps:
        return 0
    allg = list(base) + comps
    sets = KmerSets.from_sequences([g.kmer_text() for g in allg], kmer_size, KmerType.DNA, flags, ctx)
    nb = len(base)
    if within:
        rowptr, cols, d = sets.within(max_dist, rows=(nb, len(allg)), cols=(0, nb), method=method)
        for a, g in enumerate(comps):
            for p in range(rowptr[a], rowptr[a + 1]):
                out.write(f"{g.id}\t{base[cols[p]].id}\t{java_double(d[p])}\n")
        return int(rowptr[len(comps)])
    # one rectangle: rows = comparison genomes, cols = base genomes (GenomeProcessor.java:140)
    _, D = sets.matrix((nb, len(allg)), (0, nb), method=method, want_I=False)
    n = 0
    for a, g in enumerate(comps):
        for i, bg in enumerate(base):                                             # GenomeProcessor.java:143-144
            out.write(f"{g.id}\t{bg.id}\t{java_double(D[a, i])}\n")
            n += 1
    return n


def java_string_hash(s: str) -> int:
    """java.lang.String.hashCode (UTF-16 code units, int32 wrap-around)."""
    b = s.encode("utf-16-be")
    h = 0
    for i in range(0, len(b), 2):
        h = (31 * h + ((b[i] << 8) | b[i + 1])) & 0xFFFFFFFF
    return h - (1 << 32) if h & 0x80000000 else h


def java_table_size_for(initial_capacity: int) -> int:
    """java.util.HashMap.tableSizeFor: the power of two >= initial_capacity."""
    cap = 1
    while cap < initial_capacity:
        cap *= 2
    return max(cap, 1)


def java_hashmap_order(keys: Sequence[str], initial_capacity: int = 16) -> list[int]:
    """Iteration order of a java.util.HashMap<String, V> created with
    `new HashMap<>(initial_capacity)` into which `keys` (distinct) were put in
    order: bucket (h ^ h >>> 16) & (cap - 1), cap = tableSizeFor(initial
    capacity), doubled whenever a put takes the size past 0.75 · cap;
    insertion order within a bucket (resizes split bins keeping it). The reps
    processors iterate repMap.values() in this order: distReps creates it with
    capacity 500 (DistanceRepsProcessor.java:175, iterated at :190,238),
    fastaReps with 100 (FastaDistanceRepsProcessor.java:90, iterated at :124).
    Tree bins (>= 8 keys in one bucket of a table >= 64) are not modelled."""
    n = len(keys)
    cap = java_table_size_for(initial_capacity)
    while n > cap * 3 // 4:
        cap *= 2
    def bucket(s):
        h = java_string_hash(s) & 0xFFFFFFFF
        return (h ^ (h >> 16)) & (cap - 1)
    return sorted(range(n), key=lambda i: (bucket(keys[i]), i))


#: new HashMap<String, GenomeKmers>(500), DistanceRepsProcessor.java:175
DISTREPS_REPMAP_CAPACITY = 500


def _greedy_host(sets: KmerSets, keys: Sequence[str], max_dist: float) -> list[int]:
    """Pass 1 with the reference's repMap semantics, one row query per set:
    a new representative whose key is already in repMap replaces the old one
    (HashMap.put), keeping that key's slot. Returns the representatives in
    insertion-key order (index of the set each key now maps to)."""
    rep_of_key: dict[str, int] = {}
    for i, key in enumerate(keys):
        reps = list(rep_of_key.values())
        if reps and sets.row_query(i, reps, L.QUERY_ANY_LE, max_dist):
            continue
        rep_of_key[key] = i
    return list(rep_of_key.values())


def _greedy(sets, keys: Sequence[str], max_dist: float) -> list[int]:
    """Pass 1: on the device when keys are unique (gdist_greedy_reps; on
    sketches gdist_sketch_greedy_reps), otherwise the host loop with
    HashMap.put replacement. `sets`: KmerSets or SketchSets."""
    if len(set(keys)) == len(keys):
        is_rep = sets.greedy_reps(max_dist)
        return [int(i) for i in np.flatnonzero(is_rep)]
    return _greedy_host(sets, keys, max_dist)


def _sketched(sets: KmerSets, width: int):
    """The sets' MinHash sketches of `width`; the kmer sets are freed, since
    the selection reads the signatures only."""
    try:
        return sets.sketches(width)
    finally:
        sets.free()


def fasta_reps(records: Sequence[FastaRecord], out: TextIO, kmer_size: int = 0, max_dist: float = 0.97,
               kmer_type: KmerType = KmerType.DNA, flags: int = 0, ctx: Context | None = None,
               sketch_width: int = 0) -> list[int]:
    """fastaReps (FastaDistanceRepsProcessor.java:111-149): greedy
    representatives in input order; one output line per new representative
    (a repeated label re-enters repMap under its key and is printed again).
    sketch_width > 0: the selection runs on the sequences' MinHash sketches of
    that width, d the sketch distance (0: on the kmer sets, as the reference)."""
    k = kmer_size or kmer_type.getKmerSize()
    if k < 2:
        raise ParseFailureException("Kmer size must be at least 2.")           # FastaDistanceRepsProcessor.java:84-85
    out.write("seq\tname\n")                                                  # FastaDistanceRepsProcessor.java:115
    if not records:
        return []
    sets = KmerSets.from_sequences([r.sequence for r in records], k, kmer_type, flags, ctx)
    if sketch_width > 0:
        sets = _sketched(sets, sketch_width)
    labels = [r.label for r in records]
    if len(set(labels)) == len(labels):
        reps = _greedy(sets, labels, max_dist)
        printed = reps
    else:
        # replayed on the host to print every put, including replacements
        printed, rep_of_key = [], {}
        for i, key in enumerate(labels):
            cur = list(rep_of_key.values())
            if cur and sets.row_query(i, cur, L.QUERY_ANY_LE, max_dist):
                continue
            rep_of_key[key] = i
            printed.append(i)
        reps = list(rep_of_key.values())
    for i in printed:
        out.write(f"{records[i].label}\t{records[i].comment}\n")            # FastaDistanceRepsProcessor.java:141-144
    return reps


def distance_reps(genomes: Sequence[Genome], kmer_size: int = 9, max_dist: float = 0.97, flags: int = 0,
                  ctx: Context | None = None, sketch_width: int = 0) -> tuple[str, str, str]:
    """distReps (DistanceRepsProcessor.java:140-275): returns (file name
    prefix, list.tbl text, stats.tbl text). Pass 1 picks representatives in
    input order; pass 2 assigns every genome its closest representative,
    ties to the earlier one in repMap's HashMap iteration order.
    sketch_width > 0: both passes run on the genomes' MinHash sketches of that
    width, d the sketch distance (0: on the kmer sets, as the reference)."""
    if kmer_size < 4:
        raise ParseFailureException("Kmer size must be at least 4.")           # DistanceRepsProcessor.java:156-157
    if max_dist <= 0.0 or max_dist >= 1.0:
        raise ParseFailureException("Distance must be strictly between 0 and 1.")  # DistanceRepsProcessor.java:160-161
    prefix = "rep%.4f_K%d" % (max_dist, kmer_size)                              # DistanceRepsProcessor.java:212
    sets = KmerSets.from_sequences([g.kmer_text() for g in genomes], kmer_size, KmerType.DNA, flags, ctx)
    if sketch_width > 0:
        sets = _sketched(sets, sketch_width)
    ids = [g.id for g in genomes]
    reps = _greedy(sets, ids, max_dist)                                         # pass 1 (DistanceRepsProcessor.java:185-200)
    rep_set = set(reps)
    # repMap iteration order (keys = genome ids, put in pass-1 order)
    order = java_hashmap_order([ids[r] for r in reps], DISTREPS_REPMAP_CAPACITY)
    ordered_reps = [reps[o] for o in order]
    lines = ["genome_id\tgenome_name\trep_id\trep_name\tdistance"]
    counts: dict[int, int] = {}
    unique = len(set(ids)) == len(ids)
    if unique and reps:
        rank = np.full(len(genomes), len(genomes), dtype=np.int64)
        for pos, r in enumerate(ordered_reps):
            rank[r] = pos
        _, rep_of, rep_d = sets.greedy_reps(max_dist, assign=True, tie_rank=rank)
    for i, g in enumerate(genomes):                                             # pass 2 (DistanceRepsProcessor.java:220-262)
        if i in rep_set:
            r, d = i, 0.0
        elif unique:
            r, d = int(rep_of[i]), float(rep_d[i])
        else:
            pos, d = sets.row_query(i, ordered_reps, L.QUERY_ARGMIN)
            r = ordered_reps[pos]
        rg = genomes[r]
        lines.append(f"{g.id}\t{g.name}\t{rg.id}\t{rg.name}\t{java_double(d)}")
        counts[r] = counts.get(r, 0) + 1
    stats = ["rep_id\trep_name\tsize"]
    for r, c in sorted(counts.items(), key=lambda kv: (-kv[1], genomes[kv[0]].id)):   # sortedCounts (DistanceRepsProcessor.java:268)
        stats.append(f"{genomes[r].id}\t{genomes[r].name}\t{c}")
    return prefix, "\n".join(lines) + "\n", "\n".join(stats) + "\n"


# ----------------------------------------------------------------- width
INVALID_TARGET_SIZE = 2**31 - 1          # Integer.MAX_VALUE, WidthProcessor.java:53


def sketch_sizes(min_size: int, max_size: int, step: int) -> list[int]:
    """SizeList.getSizes(min, max, step) (WidthProcessor.java:104; the class is
    in the absent org.theseed jar): min, min+step, ... up to max (inferred)."""
    return list(range(min_size, max_size + 1, step))


def width_process_group(group_id: str, sets: KmerSets, sizes: Sequence[int], out: TextIO,
                        target_error: float = 0.001, sweep: bool = False) -> int | None:
    """WidthProcessor.ProcessGroup (WidthProcessor.java:153-208): exact
    all-pairs on the device, then per sketch size the sketch all-pairs and the
    relative error |r - s| * 2 / (r + s) over every pair i < j whose distances
    differ, summed in the reference's i-major order; one output line per size.
    Returns the smallest size whose mean error meets the target
    (INVALID_TARGET_SIZE if none), or None for a group with no pair < 1.0.

    sweep: one sets.sketches(max(sizes)) and one KmerSets.width_sweep
    (gdist_width_sweep) answer every size, with neither table leaving the
    device. The lines are the same; the total is then the exact sum of the
    errors quantised to 2^-62 instead of the i-major fp64 sum, so a printed
    mean can differ only where it lies within ~1e-10 of a rounding boundary
    of its fourth decimal."""
    if sweep and len(sizes):
        return _width_sweep_group(group_id, sets, sizes, out, target_error)
    n = len(sets)
    _, D = sets.matrix(upper=True)
    iu = np.triu_indices(n, 1)                      # (i, j) in i-major order
    real = D[iu]
    pairs = int(np.count_nonzero(real < 1.0))
    if pairs == 0:
        return None
    min_good = INVALID_TARGET_SIZE
    for size in sizes:
        sk = sets.sketches(size)
        soff, _ = sk.download()
        dwarves = int(np.count_nonzero(np.diff(soff) < size))
        _, SD = sk.matrix(upper=True)
        s = SD[iu]
        diff = real != s
        err = np.abs(real[diff] - s[diff]) * 2.0 / (real[diff] + s[diff])
        total = float(np.cumsum(err)[-1]) if err.size else 0.0     # sequential, as `total += error`
        max_err = 0.0
        if err.size:
            m = float(np.max(err))
            max_err = m if m > 0.0 else 0.0
        mean = total / pairs
        out.write(f"{group_id}\t{size:8d}\t{pairs:8d}\t{dwarves:8d}\t{java_format_f(mean, 8, 4)}\t"
                  f"{java_format_f(max_err, 8, 4)}\n")
        if size < min_good and mean <= target_error:
            min_good = size
    return min_good


def _width_sweep_group(group_id: str, sets: KmerSets, sizes: Sequence[int], out: TextIO,
                       target_error: float) -> int | None:
    """width_process_group over one width_sweep call: the same lines and the
    same min_good logic."""
    sizes = list(sizes)
    sk = sets.sketches(max(sizes))
    try:
        # a call takes at most WIDTH_MAX_SIZES sizes: a longer list goes in parts
        parts = [sets.width_sweep(sk, sizes[c:c + L.WIDTH_MAX_SIZES])
                 for c in range(0, len(sizes), L.WIDTH_MAX_SIZES)]
    finally:
        sk.free()
    pairs = parts[0].pairs
    if pairs == 0:
        return None
    min_good = INVALID_TARGET_SIZE
    for res in parts:
        for k in range(len(res)):
            size, mean, max_err = int(res.size[k]), float(res.mean[k]), float(res.max_err[k])
            out.write(f"{group_id}\t{size:8d}\t{pairs:8d}\t{int(res.dwarves[k]):8d}\t{java_format_f(mean, 8, 4)}\t"
                      f"{java_format_f(max_err, 8, 4)}\n")
            if size < min_good and mean <= target_error:
                min_good = size
    return min_good


def width_processor(rows: Iterable[tuple[str, str]], min_size: int, max_size: int, out: TextIO,
                    step: int = 10, max_group: int = 1000, target_error: float = 0.001, kmer_size: int = 8,
                    ctx: Context | None = None, sweep: bool = False) -> int:
    """WidthProcessor (width): `rows` are (group id, protein sequence) in input
    order; consecutive rows of one group form a group, split at max_group
    (WidthProcessor.java:117-131). Validation as validateParms
    (WidthProcessor.java:88-106). Returns the target sketch size (the largest
    per-group minimum, INVALID_TARGET_SIZE when some group had none). sweep:
    every group through one width_sweep call (width_process_group)."""
    if min_size > max_size:
        raise ParseFailureException("Minimum sketch size cannot be larger than maximum.")
    if step <= 0:
        raise ParseFailureException("Step size must be greater than 0.")
    if max_group < 10:
        raise ParseFailureException("Maximum group size must be 10 or greater.")
    if target_error > 0.1 or target_error <= 0.0:
        raise ParseFailureException("Target error must be > 0 and < 0.1.")
    sizes = sketch_sizes(min_size, max_size, step)
    target = min_size
    out.write("Group\tSize\tPairs\tDwarves\tMean E\tMax E\n")

    def flush(gid, prots):
        nonlocal target
        sets = KmerSets.from_sequences(prots, kmer_size, KmerType.PROT, 0, ctx)
        good = width_process_group(gid, sets, sizes, out, target_error, sweep)
        if good is not None and good > target:
            target = good

    group_id, prots = "", []
    for gid, seq in rows:
        if gid != group_id or len(prots) >= max_group:
            if prots:
                flush(group_id, prots)
            group_id, prots = gid, []
        prots.append(seq)
    if prots:
        flush(group_id, prots)
    return target


def closest_genomes(queries: Sequence[Genome], subjects: Sequence[Genome], out: TextIO, kmer_size: int = 21,
                    neighbors: int = 10, max_dist: float = 0.9, flags: int = 0,
                    ctx: Context | None = None) -> tuple[int, int, int]:
    """The `mash` table answered exactly: for every query genome its `neighbors`
    closest subject genomes within `max_dist` by kmer (Jaccard) distance, over
    every subject instead of the LSH buckets of MashProcessor.java:150 (defaults
    MashProcessor.java:104-106). Subjects and queries are packed as one
    collection and one KmerSets.closest call takes the queries as rows and the
    subjects as columns. The header is MashProcessor.java:144 and each row
    MashProcessor.java:161; as the reference does, a row prints the SUBJECT id
    and name first, then the query's, under a header that names the query
    first. Rows of one query are nearest first (ties by subject order). Returns
    (queries, neighbours found, searches with none), the counters of
    MashProcessor.java:168."""
    # the header of MashProcessor.java:144
    out.write("query_id\tquery_name\tsubject_id\tsubject_name\tdistance\n")
    nq, ns = len(queries), len(subjects)
    if nq == 0:
        return 0, 0, 0
    if ns == 0:
        return nq, 0, nq
    allg = list(subjects) + list(queries)
    sets = KmerSets.from_sequences([g.kmer_text() for g in allg], kmer_size, KmerType.DNA, flags, ctx)
    idx, d, cnt = sets.closest(neighbors, max_dist, rows=(ns, ns + nq), cols=(0, ns))
    found = none = 0
    for a, q in enumerate(queries):
        if cnt[a] == 0:
            none += 1
            continue
        for r in range(cnt[a]):
            s = subjects[int(idx[a, r])]
            # "%s\t%s\t%s\t%s\t%8.3f%n" of MashProcessor.java:161: subject first
            out.write(f"{s.id}\t{s.name}\t{q.id}\t{q.name}\t{java_format_f(float(d[a, r]), 8, 3)}\n")
            found += 1
    return nq, found, none


def find_genomes(db: "KmerSets | SketchSets", subjects: Sequence[Genome], queries: Iterable[Genome], out: TextIO,
                 neighbors: int = 10, max_dist: float = 0.9, batch: int = 64, kmer_size: int | None = None,
                 kmer_type: KmerType = KmerType.DNA, flags: int = 0) -> tuple[int, int]:
    """The `find` table over a resident database: `db` holds the kmer sets of
    `subjects` (set j is subjects[j]) and stays on the device as it is, as the
    reference loads its genome database once and then answers one getClosest
    per incoming genome. The queries are packed `batch` at a time with the
    database's k and pack flags and go through KmerSets.cross_closest; the
    database is never packed again. Neighbours are exact (every subject, not
    the LSH buckets), nearest first, ties by subject order. The neighbour's id
    and name are one field with a tab inside, as the database returns them.
    Returns (neighbours found, searches with none), the counters of the
    reference's closing log line.

    `db` may be a SketchSets (the reference's MinHash database): the queries
    are then packed with kmer_size, kmer_type and flags (the spec the
    database's sketches were made from; read for a sketch database only),
    sketched to the database's width and go through SketchSets.cross_closest,
    SKETCH_JACCARD and EMPTY_NAN of `flags` passed on to it."""
    # the database loaded once, one getClosest per genome: FindProcessor.java:94-110
    # defaults (10 neighbours, 0.9): FindProcessor.java:72-73
    # the header: FindProcessor.java:100
    out.write("genome_id\tgenome_name\tneighbor_id\tneighbor_name\tdistance\n")
    if len(db) != len(subjects):
        raise ValueError(f"the database holds {len(db)} sets but {len(subjects)} subjects were named")
    if batch < 1:
        raise ValueError("batch must be at least 1")
    sketched = isinstance(db, SketchSets)
    if sketched and kmer_size is None:
        raise ValueError("a sketch database needs the kmer_size its sketches were made with")
    found = fail = 0

    def closest_of(group):
        texts = [g.kmer_text() for g in group]
        if not sketched:
            qs = db.pack_like(texts)
            try:
                return db.cross_closest(qs, neighbors, max_dist)
            finally:
                qs.free()
        pack_flags = flags & ~(L.SKETCH_JACCARD | L.EMPTY_NAN)
        ks = KmerSets.from_sequences(texts, kmer_size, kmer_type, pack_flags, db.ctx)
        try:
            qs = ks.sketches(db.info()[1])
        finally:
            ks.free()
        try:
            return db.cross_closest(qs, neighbors, max_dist, flags=flags & (L.SKETCH_JACCARD | L.EMPTY_NAN))
        finally:
            qs.free()

    def flush(group):
        nonlocal found, fail
        idx, d, cnt = closest_of(group)
        for a, q in enumerate(group):
            # no neighbour counts as a failure: FindProcessor.java:111
            if cnt[a] == 0:
                fail += 1
            for r in range(cnt[a]):
                s = subjects[int(idx[a, r])]
                # the row format "%s\t%s\t%s\t%8.3f%n": FindProcessor.java:113-114
                out.write(f"{q.id}\t{q.name}\t{s.id}\t{s.name}\t{java_format_f(float(d[a, r]), 8, 3)}\n")
                found += 1

    group = []
    for g in queries:
        group.append(g)
        if len(group) >= batch:
            flush(group)
            group = []
    if group:
        flush(group)
    # the counters of the closing log line: FindProcessor.java:119
    return found, fail


def genomes_against(db: KmerSets, base: Sequence[Genome], comparisons: Iterable[Genome], out: TextIO,
                    max_dist: float = 0.9, within: bool = False, batch: int = 64) -> int:
    """The `genomes` table over a resident base collection: `db` holds the kmer
    sets of `base` (set j is base[j]) and stays on the device as it is, as the
    reference pre-loads its base genomes and then compares every comparison
    genome against them (GenomeProcessor.java:100-111,140). The comparison
    genomes are packed `batch` at a time with the database's k and pack flags;
    the base genomes are never packed again. The header and the lines are
    those of genome_distance for the same genomes: every pair
    (KmerSets.cross_matrix), or with within=True only the pairs with distance
    <= max_dist, the documented -m filter (GenomeProcessor.java:35), from
    KmerSets.cross_within. Returns the lines written."""
    if max_dist <= 0.0 or max_dist > 1.0:
        raise ParseFailureException("Maximum distance must be > 0 and <= 1.")    # GenomeProcessor.java:89-90
    if len(db) != len(base):
        raise ValueError(f"the database holds {len(db)} sets but {len(base)} base genomes were named")
    if batch < 1:
        raise ValueError("batch must be at least 1")
    out.write("genome1\tgenome2\tdistance\n")                                    # GenomeProcessor.java:121
    if not base:
        return 0
    n = 0

    def flush(group):
        nonlocal n
        qs = db.pack_like([g.kmer_text() for g in group])
        try:
            if within:
                rowptr, cols, d = db.cross_within(qs, max_dist)
            else:
                _, D = db.cross_matrix(qs, want_I=False)
        finally:
            qs.free()
        for a, g in enumerate(group):
            if within:
                for p in range(rowptr[a], rowptr[a + 1]):
                    out.write(f"{g.id}\t{base[cols[p]].id}\t{java_double(d[p])}\n")
                n += int(rowptr[a + 1] - rowptr[a])
            else:
                for i, bg in enumerate(base):                                     # GenomeProcessor.java:143-144
                    out.write(f"{g.id}\t{bg.id}\t{java_double(D[a, i])}\n")
                n += len(base)

    group = []
    for g in comparisons:
        group.append(g)
        if len(group) >= batch:
            flush(group)
            group = []
    if group:
        flush(group)
    return n


def group_labels(ids: Sequence[str], groupings: dict) -> tuple[list[str], np.ndarray]:
    """(type names, int32 labels [T, N]) of `groupings` (type name -> {genome id
    -> group id}) for the sets `ids`: group ids become integers by first
    appearance along `ids`, a genome the grouping does not hold becomes -1
    (the null group of GroupTypeSpec.java:78-80)."""
    names = list(groupings)
    lab = np.full((len(names), len(ids)), -1, dtype=np.int32)
    for t, name in enumerate(names):
        gmap, seen = groupings[name], {}
        for i, gid in enumerate(ids):
            grp = gmap.get(gid)
            if grp is not None:
                lab[t, i] = seen.setdefault(grp, len(seen))
    return names, lab


def write_distance_check(stats, names: Sequence[str], out: TextIO, name: str, header: bool = True) -> int:
    """The distCheck table of one distance source `name` from a GroupStats: an
    `in` and an `out` row per grouping (DistanceCheckProcessor.java:180-181),
    doubles as Java prints them, `ones` an int. A side without a value below
    1.0 prints 1.0 five times (DistanceCheckProcessor.java:203-209); low and
    high are mean -/+ sdev in fp64 (DistanceCheckProcessor.java:216-218).
    Returns the bad pairs over all groupings (DistanceCheckProcessor.java:185)."""
    if header:
        # the header of DistanceCheckProcessor.java:151
        out.write("dist_file\tgroup_type\tin_out\tmin\tlow\tmean\thigh\tmax\tones\n")
    low, high = stats.low, stats.high
    for t, gtype in enumerate(names):
        for k, side in enumerate(("in", "out")):
            if stats.n[t, k] == 0:
                vals = [1.0] * 5
            else:
                vals = [stats.min[t, k], low[t, k], stats.mean[t, k], high[t, k], stats.max[t, k]]
            # the row of DistanceCheckProcessor.java:221-222
            cells = [name, gtype, side] + [java_double(float(v)) for v in vals] + [str(int(stats.ones[t, k]))]
            out.write("\t".join(cells) + "\n")
    return int(stats.bad.sum())


def distance_check(sets, ids: Sequence[str], groupings: dict, out: TextIO, name: str, header: bool = True,
                   **kw) -> int:
    """distCheck (DistanceCheckProcessor.java:149-223) over the distances of a
    device-resident collection instead of a distance file: which grouping the
    distance predicts best. `sets` is a KmerSets or SketchSets whose set i is
    genome ids[i]; `groupings` maps a type name to {genome id -> group id};
    **kw goes to group_stats (rows, cols, upper, method, flags; by default the
    pairs j > i, each pair once as a distance file lists them). min, max, ones
    and the counts equal the reference's on the same pairs; its mean and sd
    come from an incremental update in file order and may differ from these
    exactly rounded ones in the last digits. Returns the bad pairs."""
    if len(ids) != len(sets):
        raise ValueError(f"{len(ids)} ids for {len(sets)} sets")
    names, lab = group_labels(ids, groupings)
    return write_distance_check(sets.group_stats(lab, **kw), names, out, name, header)


def distance_distribution(sets, ids: Sequence[str], groupings: dict, out: TextIO, name: str, buckets: int = 50,
                          header: bool = True, **kw) -> int:
    """The --dist companion of distance_check: how the in-group and out-group
    distances of every grouping are distributed over `buckets` equal buckets of
    [0, 1] (TaxCheckProcessor.java:93 sets up 50 of them,
    TaxCheckProcessor.java:133-135 feeds every series of distances in), from
    one histogram call over a device-resident collection. The edges are
    i / buckets, i = 0..buckets; one row per (grouping, in / out, bucket) with
    the columns dist_file, group_type, in_out, low, high, count: the bucket
    low <= d < high, doubles as Java prints them. The last row of a series is
    d >= 1.0 and has `high` empty; d < 0.0 never occurs and has no row; NaN
    distances are in no bucket. The reference writes its buckets to an Excel
    sheet, this writes the same counts as a table. **kw goes to histogram
    (rows, cols, upper, method, flags; by default the pairs j > i). Returns
    the bad pairs."""
    if len(ids) != len(sets):
        raise ValueError(f"{len(ids)} ids for {len(sets)} sets")
    if not 1 <= buckets <= 1022:
        raise ValueError(f"{buckets} buckets: 1 .. 1022")
    names, lab = group_labels(ids, groupings)
    edges = np.array([i / buckets for i in range(buckets + 1)], dtype=np.float64)
    hist = sets.histogram(edges, lab, **kw)
    if header:
        out.write("dist_file\tgroup_type\tin_out\tlow\thigh\tcount\n")
    for t, gtype in enumerate(names):
        for k, side in enumerate(("in", "out")):
            for b in range(1, len(edges) + 1):
                high = java_double(float(edges[b])) if b < len(edges) else ""
                cells = [name, gtype, side, java_double(float(edges[b - 1])), high, str(int(hist.counts[2 * t + k, b]))]
                out.write("\t".join(cells) + "\n")
    return int(hist.bad.sum())
