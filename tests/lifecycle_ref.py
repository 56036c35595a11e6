"""Host model of a collection whose state changes between calls (append,
concat, bitset build, prepare, release_codes): numpy and the CPU oracle, no
call into the library. Shared by test_lifecycle_host.py (CPU) and
test_gpu_lifecycle.py.

A fixed pool of sequences per kmer spec is packed by the oracle once per
process, with its whole pool x pool I / D. A model collection is a list of
pool indices (an index may repeat: exact duplicates); its expected CSR is the
pool's per-set codes in that order, its expected matrices are
D_pool[np.ix_(idx, idx)]. walk(seed, steps) is a deterministic list of
operations over such a model; it only produces operations, the GPU test's
driver applies them to a real handle.
"""
import functools

import numpy as np

import closest_ref
import group_ref

SPECS = {"dna": dict(kind=0, k=15, flags=0)}

MUTATIONS = ("append", "append_empty", "concat", "build", "prepare_auto", "release")
CONSUMERS = ("matrix_sorted", "matrix_bitset", "matrix_auto", "device_steps_x3", "row_query_all", "any_le",
             "argmin", "closest", "group_stats", "greedy_reps", "sketch_matrix")
NEEDS_CODES = ("matrix_sorted", "sketch_matrix")      # refused once the codes are released
SEEDS = (0, 1, 2, 3, 4)
STEPS = 25
N_REL, N_LONG = 150, 4
SKETCH_WIDTHS = (64, 200)


def legal_pairs():
    """Every (mutation kind, consumer kind) a walk may hold: a released
    collection cannot answer the consumers that read codes."""
    return [(m, c) for m in MUTATIONS for c in CONSUMERS if not (m == "release" and c in NEEDS_CODES)]


def sequences(spec="dna"):
    """The pool: 150 related sets, 3 exact duplicates, 40 unrelated, an empty
    sequence, one shorter than k, one with a 0-byte contig separator inside,
    4 long ones of 30 kbp (about ten times the median set)."""
    from gdist import synth
    assert spec == "dna"
    rel = [bytes(r) for r in synth.genomes(N_REL, 3000, 0.08, 51)]
    dup = [rel[5], rel[5], rel[77]]
    unrel = [bytes(synth.genomes(1, 3000, 0.0, 200 + i)[0]) for i in range(40)]
    contigs = rel[3][:1400] + b"\0" + rel[9][1400:]
    long_ = [bytes(r) for r in synth.genomes(N_LONG, 30000, 0.03, 52)]
    return rel + dup + unrel + [b"", b"ACGTACGTAC", contigs] + long_


class Pool:
    def __init__(self, spec):
        import oracle
        s = SPECS[spec]
        self.spec, self.kind, self.k, self.flags = spec, s["kind"], s["k"], s["flags"]
        self.seqs = sequences(spec)
        self.n = len(self.seqs)
        self.off, self.codes = oracle.pack(self.seqs, self.k, self.kind, self.flags)
        self.sets = [self.codes[self.off[i]:self.off[i + 1]] for i in range(self.n)]
        self.sizes = np.diff(self.off)
        self.I, self.D = oracle.matrix(self.off, self.codes, 0, self.n, 0, self.n, flags=0, nthreads=8)
        for a in (self.off, self.codes, self.sizes, self.I, self.D):
            a.setflags(write=False)

    def csr(self, idx):
        """(offsets, codes) of the collection holding the pool's sets `idx`, in that order."""
        off = np.zeros(len(idx) + 1, dtype=np.int64)
        if len(idx):
            off[1:] = np.cumsum(self.sizes[list(idx)])
        codes = np.concatenate([self.sets[i] for i in idx]) if len(idx) else np.zeros(0, np.uint64)
        return off, codes.astype(np.uint64)

    def matrices(self, idx):
        ix = np.asarray(list(idx), dtype=np.int64)
        return self.I[np.ix_(ix, ix)], self.D[np.ix_(ix, ix)]


@functools.lru_cache(maxsize=None)
def pool(spec="dna"):
    """The spec's pool with the oracle's pack and whole matrix, once per process. Read-only."""
    return Pool(spec)


@functools.lru_cache(maxsize=None)
def pool_sketches(spec, width):
    """The oracle's bottom-`width` signature of every pool set."""
    import oracle
    p = pool(spec)
    return [oracle.sketch(c, p.k, p.kind, width) for c in p.sets]


@functools.lru_cache(maxsize=None)
def pool_sketch_matrix(spec, width, flags):
    """The oracle's sketch (common, distance) of every ordered pair of the pool."""
    import oracle
    sig = pool_sketches(spec, width)
    n = len(sig)
    Cm, Dm = np.zeros((n, n), np.int32), np.zeros((n, n), np.float64)
    for i in range(n):
        for j in range(n):
            Dm[i, j], Cm[i, j] = oracle.sketch_distance(sig[i], sig[j], width, flags)
    Cm.setflags(write=False)
    Dm.setflags(write=False)
    return Cm, Dm


# ---------------------------------------------------------------- expected answers
def any_le_ref(drow, t):
    """GDIST_QUERY_ANY_LE: some listed distance <= t (a t equal to a distance hits)."""
    return bool(any(float(d) <= t for d in drow))


def argmin_ref(drow):
    """GDIST_QUERY_ARGMIN: (position in the column list, distance) of the
    smallest distance strictly below 1.0, ties to the lowest position (a
    repeated column is found at its first place); (-1, 1.0) when none."""
    bi, bd = -1, 1.0
    for c, d in enumerate(drow):
        if float(d) < bd:
            bi, bd = c, float(d)
    return bi, bd


def greedy_ref(D, t):
    """(reps, rep_of, rep_d): the sequential loop of gdist_greedy_reps over D;
    pass 2 with the default tie rank (index), d < 1.0 only."""
    n = len(D)
    reps = []
    for k in range(n):
        if not any(D[k, r] <= t for r in reps):
            reps.append(k)
    rep_of, rep_d = np.full(n, -1, np.int64), np.ones(n, np.float64)
    isrep = set(reps)
    for k in range(n):
        if k in isrep:
            rep_of[k], rep_d[k] = k, 0.0
            continue
        cand = [r for r in reps if D[k, r] < 1.0]
        if cand:
            best = min(cand, key=lambda r: (D[k, r], r))
            rep_of[k], rep_d[k] = best, D[k, best]
    return reps, rep_of, rep_d


def labels_of(idx):
    """Two groupings of a model collection, from the pool indices alone (so
    duplicates share their groups): residues, and blocks with unlabelled sets."""
    pi = np.asarray(list(idx), dtype=np.int64)
    return np.stack([pi % 4, np.where(pi % 7 == 0, -1, pi // 50)]).astype(np.int32)


closest_ref_fn = closest_ref.closest_ref
group_ref_fn = group_ref.group_ref


# ---------------------------------------------------------------- the walk
def _region(rng, n):
    """A region of an n-set collection: the whole square, its upper triangle, or a rectangle."""
    kind = int(rng.integers(3))
    if kind == 0 or n < 4:
        return dict(rows=(0, n), cols=(0, n), upper=False)
    if kind == 1:
        return dict(rows=(0, n), cols=(0, n), upper=True)
    r0 = int(rng.integers(0, n - 1))
    r1 = int(rng.integers(r0 + 1, n + 1))
    c0 = int(rng.integers(0, n - 1))
    c1 = int(rng.integers(c0 + 1, n + 1))
    return dict(rows=(r0, r1), cols=(c0, c1), upper=bool(rng.integers(2)))


def _cols(rng, n, q):
    """A column list with a repeated column, the query itself and the last set."""
    cols = [int(x) for x in rng.integers(0, n, size=6)]
    return cols + [cols[1], q, n - 1, cols[0]]


def _consumer(rng, kind, p, idx):
    n = len(idx)
    op = dict(op=kind)
    if kind in ("matrix_sorted", "matrix_bitset", "matrix_auto", "group_stats"):
        op.update(_region(rng, n))
    elif kind == "device_steps_x3":
        r0 = int(rng.integers(0, max(n // 2, 1)))
        op.update(rows=(r0, int(rng.integers(r0 + 1, n + 1))))
    elif kind in ("row_query_all", "any_le", "argmin"):
        q = int(rng.integers(n))
        cols = _cols(rng, n, q)
        if kind != "row_query_all" and rng.integers(2):
            cols = [c for c in cols if idx[c] != idx[q]] or cols       # without the query and its duplicates
        op.update(q=q, cols=cols)
        if kind == "any_le":
            drow = p.D[idx[q], [idx[c] for c in cols]]
            mode = int(rng.integers(3))
            lo = float(drow.min())
            # a threshold equal to the smallest distance (hits by equality),
            # the double just below it (misses), or the median
            op["t"] = lo if mode == 0 else float(np.nextafter(lo, -np.inf)) if mode == 1 else float(np.median(drow))
    elif kind == "closest":
        op.update(n=int(rng.choice([1, 5, 70])), max_dist=float(rng.choice([0.5, 0.9, 1.0])),
                  keep_self=bool(rng.integers(2)))
        if rng.integers(2):
            reg = _region(rng, n)
            op.update(rows=reg["rows"], cols=reg["cols"])
        else:
            op.update(rows=(0, n), cols=(0, n))
    elif kind == "greedy_reps":
        D = p.D[np.ix_(idx, idx)]
        below = np.unique(D[D < 1.0])
        # a threshold that equals a distance of the collection exactly
        op["t"] = float(below[int(rng.integers(len(below)))]) if len(below) and rng.integers(2) else \
            float(rng.choice([0.3, 0.6, 0.9]))
    elif kind == "sketch_matrix":
        op.update(width=int(rng.choice(SKETCH_WIDTHS)), jaccard=bool(rng.integers(2)), upper=bool(rng.integers(2)))
    return op


def walk(seed, steps=STEPS, spec="dna"):
    """The operations of walk `seed`: lives of one collection, each opened by
    {"op": "pack", "idx"}, then `steps` pairs of one mutation and one consumer.

    Mutations: append (idx; realloc: True when the batch holds more codes
    than the collection, which no doubled buffer can take in place, False
    when it fits in the buffer the previous reallocation left, else None),
    append_empty, concat (idx of the other collection; other_first: it comes
    first), build (T, keep), prepare_auto (pairs), release. A release ends the
    life for everything that needs codes: after its consumer a new pack
    follows. Every op carries "idx": the model after it.

    The walks of SEEDS deal every legal (mutation, consumer) pair among them;
    each walk opens with an append that must reallocate and one that fits."""
    p = pool(spec)
    rng = np.random.default_rng(1000 + seed)
    pairs = legal_pairs()
    deal = np.random.default_rng(77).permutation(len(pairs))
    must = [pairs[i] for i in deal[seed % len(SEEDS)::len(SEEDS)]]
    extra = [pairs[int(i)] for i in rng.integers(0, len(pairs), size=max(steps - 2 - len(must), 0))]
    todo = must + extra
    order = rng.permutation(len(todo))
    todo = [("append", CONSUMERS[int(rng.integers(len(CONSUMERS)))]),
            ("append", CONSUMERS[int(rng.integers(len(CONSUMERS)))])] + [todo[i] for i in order]
    small = [i for i in range(p.n) if p.sizes[i] < 8000]

    ops = []
    st = dict(idx=[], total=0, cap=None)

    def pack():
        k = int(rng.integers(8, 24))
        st["idx"] = [int(x) for x in rng.choice(small, size=k, replace=False)]
        st["total"] = int(p.sizes[st["idx"]].sum())
        st["cap"] = None
        ops.append(dict(op="pack", idx=list(st["idx"])))

    pack()
    for step, (mut, cons) in enumerate(todo[:steps]):
        if len(st["idx"]) > 220:
            pack()
        idx = st["idx"]
        op = dict(op=mut)
        if mut == "append":
            if step == 0:
                # more codes than the collection holds: must reallocate
                batch = [int(x) for x in rng.choice(N_REL, size=len(idx) + 4, replace=False)] + [p.n - 1]
            elif step == 1:
                batch = [int(rng.integers(N_REL))]
            else:
                batch = [int(x) for x in rng.integers(0, p.n, size=int(rng.integers(1, 13)))]
            add = int(p.sizes[batch].sum())
            if add > st["total"]:
                op["realloc"] = True
                st["cap"] = 2 * (st["total"] + add)
            elif st["cap"] is not None and st["total"] + add <= st["cap"]:
                op["realloc"] = False
            else:
                op["realloc"] = None
                st["cap"] = None
            op["batch"] = batch
            st["idx"] = idx + batch
            st["total"] += add
        elif mut == "concat":
            other = [int(x) for x in rng.integers(0, p.n, size=int(rng.integers(0, 30)))]
            op.update(other=other, other_first=bool(rng.integers(2)))
            st["idx"] = other + idx if op["other_first"] else idx + other
            st["total"] += int(p.sizes[other].sum())
            st["cap"] = None
        elif mut == "build":
            op.update(T=int(rng.choice([-1, 0, 3, 8, 1000])), keep=bool(rng.integers(4) == 0))
        elif mut == "prepare_auto":
            op["pairs"] = float(rng.choice([-1.0, float(1 << 22)]))
        op["idx"] = list(st["idx"])
        ops.append(op)
        c = _consumer(rng, cons, p, st["idx"])
        c["idx"] = list(st["idx"])
        ops.append(c)
        if mut == "release" and step + 1 < steps:
            pack()
    return ops
