"""The lifecycle of a collection on the device: gdist_sets_append,
gdist_sets_concat and gdist_sets_release_codes change a collection under its
derived fields (dictionary, tiers, segment index, launch plans, captured
steps). After every change each consumer is compared bit for bit with the CPU
oracle: np.array_equal on codes and counts, the bits of every fp64.

The contracts of include/gdist.h pinned here: a failed append touches
nothing; an append of zero sequences changes nothing and keeps built
bitsets; a concat result is a deep copy that carries its first input's pack
flags (an uploaded collection appends with the default ones).
test_lifecycle_host.py proves on the CPU what the fixtures and the walks
below are relied on for."""
import functools
import json
import os

import numpy as np
import pytest

import lifecycle_ref as LR
import oracle

pytestmark = pytest.mark.gpu

GOLDEN = os.path.join(os.path.dirname(__file__), "golden", "kmer_golden.json")


def golden_cases():
    with open(GOLDEN) as f:
        return json.load(f)["cases"]


def golden_case(name):
    return next(c for c in golden_cases() if c["name"] == name)


def bits_equal(a, b):
    a = np.ascontiguousarray(a, np.float64)
    b = np.ascontiguousarray(b, np.float64)
    return a.shape == b.shape and np.array_equal(a.view(np.uint64), b.view(np.uint64))


def as_bytes(seqs):
    return [s if isinstance(s, bytes) else s.encode("latin-1") for s in seqs]


def upper_mask(r0, r1, c0, c1):
    return np.fromfunction(lambda a, b: (c0 + b) > (r0 + a), (r1 - r0, c1 - c0))


def check_matrix(sets, eI, eD, method, rows=None, cols=None, upper=False, tag=None):
    """sets.matrix over the region against eI / eD, the oracle's whole N x N."""
    n = len(eI)
    r0, r1 = rows or (0, n)
    c0, c1 = cols or (0, n)
    I, D = sets.matrix((r0, r1), (c0, c1), upper=upper, method=method)
    xI, xD = eI[r0:r1, c0:c1], eD[r0:r1, c0:c1]
    if upper:
        m = upper_mask(r0, r1, c0, c1)
        I, D, xI, xD = I[m], D[m], xI[m], xD[m]
    assert np.array_equal(I, xI), (tag, method, rows, cols, upper)
    assert bits_equal(D, xD), (tag, method, rows, cols, upper)


def check_all_methods(sets, eI, eD, tag=None, methods=(1, 2, 0)):
    for method in methods:
        check_matrix(sets, eI, eD, method, tag=tag)
        check_matrix(sets, eI, eD, method, upper=True, tag=tag)


def check_csr(sets, off, codes, tag=None):
    assert len(sets) == len(off) - 1, tag
    assert np.array_equal(sets.sizes(), np.diff(off)), tag
    goff, gcodes = sets.download()
    assert np.array_equal(goff, off) and np.array_equal(gcodes, codes), tag


def device_steps(ctx, sets, eI, eD, rows, ncols, bufs, calls=3, tag=None):
    """The region rows x (0, ncols), upper triangle, METHOD_BITSET, `calls`
    times into the same two device buffers (ld = ncols), poisoned before every
    call: the first call of a region runs plain and builds its plan, the
    second is captured, the rest replay the captured step."""
    import gdist
    r0, r1 = rows
    nr = r1 - r0
    dI, dD = bufs
    m = upper_mask(r0, r1, 0, ncols)
    pI, pD = np.full(nr * ncols, -7, np.int32), np.full(nr * ncols, 42.5)
    for call in range(calls):
        dI.from_host(pI)
        dD.from_host(pD)
        sets.matrix_device(dI.ptr, dD.ptr, ncols, (r0, r1), (0, ncols), upper=True, method=gdist.METHOD_BITSET)
        I = dI.to_host(np.int32, nr * ncols).reshape(nr, ncols)
        D = dD.to_host(np.float64, nr * ncols).reshape(nr, ncols)
        assert np.array_equal(I[m], eI[r0:r1, :ncols][m]), (tag, call)
        assert bits_equal(D[m], eD[r0:r1, :ncols][m]), (tag, call)
        assert np.all(I[~m] == -7) and np.all(D[~m] == 42.5), (tag, call)      # j <= i left untouched


def oracle_full(seqs, k, kind, flags):
    off, codes = oracle.pack(as_bytes(seqs), k, kind, flags)
    n = len(seqs)
    eI, eD = oracle.matrix(off, codes, 0, n, 0, n, flags=0, nthreads=8)
    return off, codes, eI, eD


def ktype(kind):
    import gdist
    return gdist.KmerType.DNA if kind == 0 else gdist.KmerType.PROT


def pool_sets(ctx, idx, p=None):
    import gdist
    p = p or LR.pool("dna")
    return gdist.KmerSets.from_sequences([p.seqs[i] for i in idx], p.k, ktype(p.kind), p.flags, ctx)


# ---------------------------------------------------------------- a. append keeps the kmer spec
@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_append_keeps_the_kmer_spec(ctx, opts, case):
    """A collection packed from the first half of a golden case and appended
    to twice is the golden case: gdist_sets_append packs with the collection's
    own kind, k and flags (strand, ambiguity, case folding, the 5-bit protein
    alphabet, contig separators), whatever the pack's chunking."""
    import gdist
    seqs, kt = case["seqs"], ktype(case["kind"])
    half = len(seqs) // 2
    rest = seqs[half:]
    cut = len(rest) // 2
    for chunked in (False, True):
        if chunked:
            opts(pack_chunk=1000, pack_codes_budget=0)
        sets = gdist.KmerSets.from_sequences(seqs[:half], case["k"], kt, case["flags"], ctx)
        assert sets.append(rest[:cut]) == half
        assert sets.append(rest[cut:]) == half + cut
        off, codes = sets.download()
        assert [[str(int(x)) for x in codes[off[i]:off[i + 1]]] for i in range(len(off) - 1)] == case["codes"]
        assert sets.sizes().tolist() == case["sizes"]
        for method in (gdist.METHOD_SORTED, gdist.METHOD_BITSET):
            I, D = sets.matrix(method=method)
            assert I.tolist() == case["I"], (chunked, method)
            assert [[gdist.java_double(x) for x in r] for r in D] == case["D"], (chunked, method)
        sk = sets.sketches(case["width"])
        so, sv = sk.download()
        assert [sv[so[i]:so[i + 1]].tolist() for i in range(len(so) - 1)] == case["sketch"]
        _, SD = sk.matrix()
        assert [[gdist.java_double(x) for x in r] for r in SD] == case["sketch_D"]
        _, SJ = sk.matrix(flags=gdist.SKETCH_JACCARD)
        assert [[gdist.java_double(x) for x in r] for r in SJ] == case["sketch_D_jaccard"]
        sk.free()
        sets.free()


# ---------------------------------------------------------------- b. a failed append
@pytest.mark.parametrize("name,bad", [("dna_keep_k6", b"ACGTX"), ("prot_k10_5bit", b"ACD1EFGHIKLM")])
def test_failed_append_changes_nothing(ctx, name, bad):
    """Contract (a) of gdist_sets_append: a batch with an unencodable sequence
    is EINVAL before anything of the collection is touched: codes, nsets, the
    built dictionary and both matrices are as before. Contract (b): an append
    of zero sequences returns nsets and keeps the built bitsets."""
    import gdist
    case = golden_case(name)
    seqs, k, kind, flags = as_bytes(case["seqs"]), case["k"], case["kind"], case["flags"]
    off, codes, eI, eD = oracle_full(seqs, k, kind, flags)
    sets = gdist.KmerSets.from_sequences(seqs, k, ktype(kind), flags, ctx)
    sets.build_bitsets(rare_threshold=3)

    def state():
        o, c = sets.download()
        return (len(sets), o.tobytes(), c.tobytes(), sets.bitset_info(), sets.rare_info(),
                [a.tobytes() for m in (gdist.METHOD_BITSET, gdist.METHOD_SORTED) for a in sets.matrix(method=m)])

    before = state()
    assert before[3][0] >= 0, "a dictionary is built (-1: none)"
    check_all_methods(sets, eI, eD, "before")
    valid = seqs[0][::-1]
    with pytest.raises(ValueError):
        oracle.kmer_codes(bad, k, kind, flags)                # the oracle refuses the sequence too
    with pytest.raises(ValueError):
        sets.append([valid, bad])
    assert state() == before
    assert sets.append([]) == len(seqs)
    assert state() == before                                  # the old dictionary, not a silently rebuilt one
    assert sets.append([valid, b""]) == len(seqs)
    off2, codes2, eI2, eD2 = oracle_full(seqs + [valid, b""], k, kind, flags)
    check_csr(sets, off2, codes2)
    check_all_methods(sets, eI2, eD2, "after")
    sets.free()


# ---------------------------------------------------------------- c. an append drops every tier
@functools.lru_cache(maxsize=None)
def shared_ancestor_case(n):
    """One ancestor, independent substitutions (the shape of test_gpu_variant's
    collection) at n sets, with the oracle's whole matrix."""
    from gdist import synth
    seqs = [bytes(r) for r in synth.genomes(n, 4000, 0.03, 41)]
    return (seqs,) + oracle_full(seqs, 21, 0, 0)


TIER_N = 256
TIERS = {
    # options, build arguments, the tier's getter, whether the threshold is explicit
    "two_tier": (dict(variant=0), dict(rare_threshold=3), lambda s: s.rare_info()[1], True),
    "keep_singletons": (dict(), dict(keep_singletons=True), lambda s: s.bitset_info()[0], True),
    "sparse": (dict(sparse_zmax=100000), dict(), lambda s: s.sparse_info()[0], False),
    "variant": (dict(variant=1, rare_t=3, variant_dmin=TIER_N // 10), dict(rare_threshold=3),
                lambda s: s.variant_info()[0], True),
    "grouped_rare": (dict(variant=0, rare_group=1), dict(), lambda s: s.variant_info()[0], True),
}


@pytest.mark.parametrize("tier", list(TIERS))
def test_append_drops_every_tier(ctx, opts, tier):
    """A collection built with one tier forced, queried (plans, a captured and
    replayed step), then appended to with related sets (pruned singletons
    become shared, rare kmers cross the threshold): nothing of the old tiers
    survives. Every whole matrix is exact, the same region into the same
    device buffers is exact three more times (the captured step's key holds
    nothing that an append changes, so a step that outlived its tiers would be
    replayed here), and the rebuilt tiers count what a collection packed in
    one go counts."""
    import gdist
    o, build, getter, explicit = TIERS[tier]
    if tier == "sparse":
        from test_gpu_parity import sparse_case
        case = sparse_case()
        seqs, eI, eD = case["seqs"], case["eI"], case["eD"]
    else:
        seqs, _, _, eI, eD = shared_ancestor_case(TIER_N)
    n = len(seqs)
    n0 = n - 24
    opts(**o)
    sets = gdist.KmerSets.from_sequences(seqs[:n0], 21, gdist.KmerType.DNA, 0, ctx)
    sets.build_bitsets(**build)
    assert getter(sets) > 0, tier
    if tier == "grouped_rare":
        assert sets.variant_layout()[:2] == (16, 4) and sets.rare_info()[1] == 0
    check_matrix(sets, eI[:n0, :n0], eD[:n0, :n0], gdist.METHOD_BITSET, upper=True, tag=tier)
    rows = (5, 69)
    bufs = (ctx.alloc(64 * n0 * 4), ctx.alloc(64 * n0 * 8))
    device_steps(ctx, sets, eI, eD, rows, n0, bufs, tag=(tier, "before"))
    at = n0
    for size in (1, 7, 16):
        assert sets.append(seqs[at:at + size]) == at
        at += size
    assert at == n and len(sets) == n and sets.bitset_info() == (-1, 0)
    if build:
        sets.build_bitsets(**build)          # a given threshold / kept singletons are arguments of the build
    for method in (gdist.METHOD_BITSET, gdist.METHOD_AUTO, gdist.METHOD_SORTED):
        check_matrix(sets, eI, eD, method, tag=(tier, "after"))
    assert getter(sets) > 0, tier
    device_steps(ctx, sets, eI, eD, rows, n0, bufs, tag=(tier, "after"))
    if explicit:
        fresh = gdist.KmerSets.from_sequences(seqs, 21, gdist.KmerType.DNA, 0, ctx)
        fresh.build_bitsets(**build)
        assert fresh.bitset_info()[0] == sets.bitset_info()[0]
        assert fresh.rare_info() == sets.rare_info() and fresh.rare_stats() == sets.rare_stats()
        assert fresh.variant_info() == sets.variant_info()
        fresh.free()
    for b in bufs:
        b.free()
    sets.free()


# ---------------------------------------------------------------- d. the segment index across an append
@pytest.mark.parametrize("state", ["one_segment", "splitters", "no_index"])
def test_append_segment_index_states(ctx, state):
    """The three states gdist_sets_append tells apart: an index of one segment
    (every set below a segment's target; the appended 30 kbp set is walked in
    sub-blocks of that one segment), an index with splitters (the new rows use
    the old splitters), and no index at all (only bitsets were built and
    used; the sorted call after the append builds one over every set)."""
    import gdist
    from gdist import synth
    length = 800 if state == "one_segment" else 6000
    base = [bytes(r) for r in synth.genomes(10, length, 0.03, 141)]
    big = bytes(synth.genomes(1, 30000, 0.03, 142)[0])
    batch = [big, b"", base[2][:length // 2] + big[:700]]
    sets = gdist.KmerSets.from_sequences(base, 21, gdist.KmerType.DNA, 0, ctx)
    _, _, bI, bD = oracle_full(base, 21, 0, 0)
    if state == "no_index":
        sets.build_bitsets()
        check_matrix(sets, bI, bD, gdist.METHOD_BITSET, tag=state)
    else:
        assert (sets.sizes().max() < 2048) == (state == "one_segment")
        check_matrix(sets, bI, bD, gdist.METHOD_SORTED, tag=state)
    assert sets.append(batch) == len(base)
    off, codes, eI, eD = oracle_full(base + batch, 21, 0, 0)
    n = len(base) + len(batch)
    check_csr(sets, off, codes, state)
    check_matrix(sets, eI, eD, gdist.METHOD_SORTED, tag=state)
    check_matrix(sets, eI, eD, gdist.METHOD_SORTED, upper=True, tag=state)
    for q in (n - 1, n - 3):
        assert bits_equal(sets.row_query(q, list(range(n))), eD[q]), (state, q)
    sets.free()


# ---------------------------------------------------------------- e. concat of kmer sets
A_IDX = list(range(60)) + [150, 160, 161, 193, 196, 197, 5, 77, 199, 170]
B_IDX = list(range(60, 100)) + [194, 5, 77, 3, 150, 171, 172, 198, 12, 13]


def check_model(sets, idx, tag=None, methods=(1, 2, 0)):
    p = LR.pool("dna")
    check_csr(sets, *p.csr(idx), tag=tag)
    eI, eD = p.matrices(idx)
    check_all_methods(sets, eI, eD, tag, methods)


def test_concat_kmer_sets(ctx):
    """gdist_sets_concat, contract (c): the result holds a's sets then b's,
    answers every method exactly, and is a deep copy: appends to an input or
    to the result do not show in the other, and the result outlives both."""
    import closest_ref
    import gdist
    import group_ref
    p = LR.pool("dna")
    na, nb = len(A_IDX), len(B_IDX)
    assert (na, nb) == (70, 50) and 194 in B_IDX and set(A_IDX) & set(B_IDX) >= {5, 77, 150}
    a, b = pool_sets(ctx, A_IDX), pool_sets(ctx, B_IDX)
    a.build_bitsets()
    aI, aD = p.matrices(A_IDX)
    check_matrix(a, aI, aD, gdist.METHOD_SORTED)             # the segment index
    res = a.concat(b)
    idx = A_IDX + B_IDX
    assert type(res) is gdist.KmerSets and res.bitset_info() == (-1, 0)
    check_csr(res, *p.csr(idx))
    eI, eD = p.matrices(idx)
    for method in (gdist.METHOD_SORTED, gdist.METHOD_BITSET, gdist.METHOD_AUTO):
        check_matrix(res, eI, eD, method, rows=(0, na), cols=(na, na + nb), tag="rectangle")
    assert int((eD[:na, na:] == 0.0).sum()) >= 5             # b's duplicates of a's sets
    for n_top, md in ((5, 0.9), (70, 1.0)):
        got = res.closest(n_top, md, rows=(0, na), cols=(na, na + nb))
        exp = closest_ref.closest_ref(eD[:na, na:], n_top, md, 0, na)
        assert np.array_equal(got[0], exp[0]) and bits_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    labels = LR.labels_of(idx)
    gs = res.group_stats(labels, rows=(0, na), cols=(na, na + nb), upper=False)
    group_ref.check_stats(gs.sides, gs.bad_raw, group_ref.group_ref(eD[:na, na:], labels, 0, na, upper=False))
    # independence
    check_model(a, A_IDX, "a after concat")
    check_model(b, B_IDX, "b after concat")
    assert a.append([p.seqs[101], p.seqs[198]]) == na
    check_model(a, A_IDX + [101, 198], "a appended")
    check_model(res, idx, "result after a's append")
    assert res.append([p.seqs[102]]) == na + nb
    check_model(res, idx + [102], "result appended")
    check_model(a, A_IDX + [101, 198], "a after the result's append")
    check_model(b, B_IDX, "b after the result's append")
    # edge shapes (a is now A_IDX + [101, 198])
    a_idx = A_IDX + [101, 198]
    empty = gdist.KmerSets.from_sequences([], p.k, gdist.KmerType.DNA, 0, ctx)
    for x, y, xi, yi in ((empty, b, [], B_IDX), (a, empty, a_idx, []), (empty, empty, [], []), (a, a, a_idx, a_idx)):
        r = x.concat(y)
        # (a collection of no sets has nothing to build a dictionary from: the default method only)
        check_model(r, xi + yi, ("edge", len(xi), len(yi)), methods=(1, 2, 0) if xi + yi else (0,))
        if x is a and y is a:
            _, D = r.matrix(rows=(0, len(a_idx)), cols=(len(a_idx), 2 * len(a_idx)), method=gdist.METHOD_BITSET)
            keep = np.array([p.sizes[i] > 0 for i in a_idx])
            assert np.all(np.diag(D)[keep] == 0.0)           # every set against its copy
        r.free()
    # refusals leave both inputs usable
    few = [p.seqs[i][:400] for i in (0, 1, 2)]
    _, _, fI, fD = oracle_full(few, 8, 0, 0)
    d8 = gdist.KmerSets.from_sequences(few, 8, gdist.KmerType.DNA, 0, ctx)
    for kind, k, flags in ((gdist.KmerType.DNA, 9, 0), (gdist.KmerType.PROT, 8, 0),
                           (gdist.KmerType.DNA, 8, gdist.STRAND_FWD), (gdist.KmerType.DNA, 8, gdist.AMBIG_SKIP)):
        other = gdist.KmerSets.from_sequences(few, k, kind, flags, ctx)      # (ACGT are amino acid letters too)
        sizes = other.sizes()
        assert len(other) == 3 and sizes.min() > 0
        with pytest.raises(ValueError):
            d8.concat(other)
        with pytest.raises(ValueError):
            other.concat(d8)
        assert np.array_equal(other.sizes(), sizes) and np.array_equal(other.download()[0][1:], np.cumsum(sizes))
        check_all_methods(d8, fI, fD, ("refused", k, flags))
        other.free()
    with pytest.raises(ValueError):
        d8.concat(b)                                                         # another k
    d8.free()
    check_model(b, B_IDX, "b after the refusals")
    # the result outlives its inputs
    a.free()
    b.free()
    empty.free()
    check_model(res, idx + [102], "result after its inputs were freed")
    res.free()


def test_concat_carries_the_first_inputs_flags(ctx):
    """Collections packed with and without case folding concatenate (their
    codes are comparable); the result equals each part packed with its own
    flags, and a later append follows the first input's. A collection from
    gdist_sets_upload appends with the default flags."""
    import gdist
    fold, nofold = golden_case("prot_k3_case_x"), golden_case("prot_k3_nofold")
    assert (fold["kind"], fold["k"], fold["flags"]) == (1, 3, 0) and nofold["flags"] == gdist.NO_CASE_FOLD
    ns = as_bytes(nofold["seqs"])
    lower = b"acdefGHIKlmacd"
    assert not np.array_equal(oracle.kmer_codes(lower, 3, 1, 0), oracle.kmer_codes(lower, 3, 1, gdist.NO_CASE_FOLD))
    for first, second in ((fold, nofold), (nofold, fold)):
        x = gdist.KmerSets.from_sequences(first["seqs"], 3, gdist.KmerType.PROT, first["flags"], ctx)
        y = gdist.KmerSets.from_sequences(second["seqs"], 3, gdist.KmerType.PROT, second["flags"], ctx)
        r = x.concat(y)
        parts = [oracle.kmer_codes(s, 3, 1, c["flags"]) for c in (first, second) for s in as_bytes(c["seqs"])]
        assert r.append([lower]) == len(parts)
        parts.append(oracle.kmer_codes(lower, 3, 1, first["flags"]))
        off = np.zeros(len(parts) + 1, np.int64)
        off[1:] = np.cumsum([len(c) for c in parts])
        codes = np.concatenate(parts).astype(np.uint64)
        check_csr(r, off, codes, first["name"])
        n = len(parts)
        eI, eD = oracle.matrix(off, codes, 0, n, 0, n)
        check_all_methods(r, eI, eD, first["name"])
        for h in (x, y, r):
            h.free()
    # uploaded codes carry no flags: the append packs with the default ones
    off, codes = oracle.pack(ns, 3, 1, gdist.NO_CASE_FOLD)
    up = gdist.KmerSets.from_codes(off, codes, 3, gdist.KmerType.PROT, ctx)
    assert up.append([lower]) == len(ns)
    add = oracle.kmer_codes(lower, 3, 1, 0)
    check_csr(up, np.append(off, off[-1] + len(add)), np.concatenate([codes, add]).astype(np.uint64), "uploaded")
    up.free()


# ---------------------------------------------------------------- f. concat of sketches
@pytest.mark.parametrize("width", LR.SKETCH_WIDTHS)
def test_concat_sketches(ctx, width):
    """gdist_sets_concat on sketch collections (4-byte signatures): the
    result's signatures, its sketch matrix under both distance flags, the
    exact M x N closest and an LSH index over it equal the oracle's."""
    import closest_ref
    import gdist
    p = LR.pool("dna")
    a_idx, b_idx = A_IDX[20:], B_IDX[10:]
    na, nb = len(a_idx), len(b_idx)
    ka, kb = pool_sets(ctx, a_idx), pool_sets(ctx, b_idx)
    A, B = ka.sketches(width), kb.sketches(width)
    assert not hasattr(gdist.SketchSets, "append")
    res = A.concat(B)
    assert type(res) is gdist.SketchSets and len(res) == na + nb
    idx = a_idx + b_idx
    sig = [LR.pool_sketches("dna", width)[i] for i in idx]
    so, sv = res.download()
    assert np.array_equal(np.diff(so), [len(s) for s in sig])
    assert np.array_equal(sv, np.concatenate(sig))
    assert any(len(s) < width for s in sig) and any(len(s) == width for s in sig)       # dwarves and full ones
    ix = np.ix_(idx, idx)
    for fl in (0, gdist.SKETCH_JACCARD):
        eC, eD = (m[ix] for m in LR.pool_sketch_matrix("dna", width, fl))
        Cm, Dm = res.matrix(rows=(0, na), cols=(na, na + nb), flags=fl)
        assert np.array_equal(Cm, eC[:na, na:]) and bits_equal(Dm, eD[:na, na:]), fl
        Cm, Dm = res.matrix(flags=fl)
        assert np.array_equal(Cm, eC) and bits_equal(Dm, eD), fl
    eD = LR.pool_sketch_matrix("dna", width, 0)[1][ix]
    got = res.closest(5, 0.95, rows=(0, na), cols=(na, na + nb))
    exp = closest_ref.closest_ref(eD[:na, na:], 5, 0.95, 0, na)
    assert np.array_equal(got[0], exp[0]) and bits_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    assert exp[2].max() == 5 and exp[2].min() < 5
    lsh = gdist.LSHIndex(res, 6, 50, seed=77)
    assert lsh.getClosest(B, 5, 0.9) == oracle.lsh_closest(sig, sig[na:], width, 6, 50, 77, 5, 0.9)
    lsh.free()
    # the inputs are untouched and independent of the result
    for s, part in ((A, sig[:na]), (B, sig[na:])):
        assert np.array_equal(s.download()[1], np.concatenate(part))
    # refusals
    other = ka.sketches(width + 1)
    for call in (lambda: A.concat(other), lambda: other.concat(A), lambda: ka.concat(A), lambda: A.concat(ka),
                 lambda: gdist.KmerSets.append(res, [b"ACGTACGTACGTACGTACGT"]),
                 lambda: gdist.KmerSets.build_bitsets(res), lambda: gdist.KmerSets.release_codes(res)):
        with pytest.raises(ValueError):
            call()
    assert np.array_equal(res.download()[1], np.concatenate(sig))
    for h in (other, res, A, B, ka, kb):
        h.free()


# ---------------------------------------------------------------- g. a released collection
def test_released_collection_on_every_consumer(ctx):
    """gdist_sets_release_codes leaves a bitsets-only collection: sizes, the
    BITSET / AUTO matrices, row queries, closest, group_stats and greedy_reps
    are exact; what needs codes (append, concat on either side, sketches, the
    sorted join, download) is EINVAL and leaves the collection answering."""
    import closest_ref
    import gdist
    import group_ref
    p = LR.pool("dna")
    idx = list(range(p.n))
    n = len(idx)
    eI, eD = p.matrices(idx)
    sets = pool_sets(ctx, idx)
    sets.build_bitsets(rare_threshold=3)
    assert sets.rare_info()[1] > 0 and sets.bitset_info()[0] > 0          # both tiers hold kmers
    sets.release_codes()
    assert len(sets) == n and np.array_equal(sets.sizes(), p.sizes)
    for method in (gdist.METHOD_BITSET, gdist.METHOD_AUTO):
        check_matrix(sets, eI, eD, method)
        check_matrix(sets, eI, eD, method, rows=(37, 150), cols=(5, 199), upper=True)
    for q in (0, 151, 193, 199):
        cols = [4, 150, 5, 199, 150, 193, q, 40]
        drow = eD[q, cols]
        assert bits_equal(sets.row_query(q, cols), drow), q
        assert sets.row_query(q, cols, gdist.QUERY_ARGMIN) == LR.argmin_ref(drow), q
        for t in (float(drow.min()), float(np.nextafter(drow.min(), -np.inf)), float(np.median(drow)), 1.0):
            assert sets.row_query(q, cols, gdist.QUERY_ANY_LE, t) == LR.any_le_ref(drow, t), (q, t)
    for method in (gdist.METHOD_AUTO, gdist.METHOD_BITSET):
        got = sets.closest(10, 0.9, method=method)
        exp = closest_ref.closest_ref(eD, 10, 0.9)
        assert np.array_equal(got[0], exp[0]) and bits_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    labels = LR.labels_of(idx)
    gs = sets.group_stats(labels)
    group_ref.check_stats(gs.sides, gs.bad_raw, group_ref.group_ref(eD, labels))
    t = float(np.quantile(eD[:150, :150], 0.2))
    reps, rep_of, rep_d = LR.greedy_ref(eD, t)
    assert 10 < len(reps) < n
    is_rep, got_of, got_d = sets.greedy_reps(t, assign=True, method=gdist.METHOD_AUTO)
    assert np.flatnonzero(is_rep).tolist() == reps and np.array_equal(got_of, rep_of) and bits_equal(got_d, rep_d)
    other = pool_sets(ctx, [0, 1, 2])
    for call in (lambda: sets.append([p.seqs[0]]), lambda: sets.append([]), lambda: sets.concat(other),
                 lambda: other.concat(sets), lambda: sets.sketches(64),
                 lambda: sets.closest(3, 0.9, method=gdist.METHOD_SORTED), lambda: sets.download(),
                 lambda: sets.matrix(method=gdist.METHOD_SORTED), lambda: sets.build_bitsets()):
        with pytest.raises(ValueError):
            call()
        assert len(sets) == n
        check_matrix(sets, eI, eD, gdist.METHOD_BITSET)
    check_model(other, [0, 1, 2], "the other side of a refused concat")
    other.free()
    sets.free()


# ---------------------------------------------------------------- h. random walks
def apply_consumer(ctx, h, op, p):
    import closest_ref
    import gdist
    import group_ref
    idx, kind = op["idx"], op["op"]
    n = len(idx)
    eI, eD = p.matrices(idx)
    if kind in ("matrix_sorted", "matrix_bitset", "matrix_auto"):
        method = {"matrix_sorted": 1, "matrix_bitset": 2, "matrix_auto": 0}[kind]
        check_matrix(h, eI, eD, method, op["rows"], op["cols"], op["upper"], tag=kind)
    elif kind == "device_steps_x3":
        nr = op["rows"][1] - op["rows"][0]
        bufs = (ctx.alloc(nr * n * 4), ctx.alloc(nr * n * 8))
        device_steps(ctx, h, eI, eD, op["rows"], n, bufs, tag=kind)
        for b in bufs:
            b.free()
    elif kind == "row_query_all":
        assert bits_equal(h.row_query(op["q"], op["cols"]), eD[op["q"], op["cols"]])
    elif kind == "any_le":
        drow = eD[op["q"], op["cols"]]
        assert h.row_query(op["q"], op["cols"], gdist.QUERY_ANY_LE, op["t"]) == LR.any_le_ref(drow, op["t"])
    elif kind == "argmin":
        assert h.row_query(op["q"], op["cols"], gdist.QUERY_ARGMIN) == LR.argmin_ref(eD[op["q"], op["cols"]])
    elif kind == "closest":
        (r0, r1), (c0, c1) = op["rows"], op["cols"]
        got = h.closest(op["n"], op["max_dist"], rows=op["rows"], cols=op["cols"], keep_self=op["keep_self"])
        exp = closest_ref.closest_ref(eD[r0:r1, c0:c1], op["n"], op["max_dist"], r0, c0, keep_self=op["keep_self"])
        assert np.array_equal(got[0], exp[0]) and bits_equal(got[1], exp[1]) and np.array_equal(got[2], exp[2])
    elif kind == "group_stats":
        (r0, r1), (c0, c1) = op["rows"], op["cols"]
        labels = LR.labels_of(idx)
        gs = h.group_stats(labels, rows=op["rows"], cols=op["cols"], upper=op["upper"])
        group_ref.check_stats(gs.sides, gs.bad_raw, group_ref.group_ref(eD[r0:r1, c0:c1], labels, r0, c0, op["upper"]))
    elif kind == "greedy_reps":
        reps, rep_of, rep_d = LR.greedy_ref(eD, op["t"])
        is_rep, got_of, got_d = h.greedy_reps(op["t"], assign=True)
        assert np.flatnonzero(is_rep).tolist() == reps
        assert np.array_equal(got_of, rep_of) and bits_equal(got_d, rep_d)
    elif kind == "sketch_matrix":
        fl = gdist.SKETCH_JACCARD if op["jaccard"] else 0
        sk = h.sketches(op["width"])
        ix = np.ix_(idx, idx)
        eC, eSD = (m[ix] for m in LR.pool_sketch_matrix(p.spec, op["width"], fl))
        Cm, Dm = sk.matrix(upper=op["upper"], flags=fl)
        m = upper_mask(0, n, 0, n) if op["upper"] else np.ones((n, n), dtype=bool)
        assert np.array_equal(Cm[m], eC[m]) and bits_equal(Dm[m], eSD[m])
        sk.free()
    else:
        raise AssertionError(kind)


@pytest.mark.parametrize("seed", LR.SEEDS)
def test_random_walk(ctx, seed):
    """lifecycle_ref.walk applied to a real handle: after every mutation len,
    sizes and (while codes are held) download equal the model, and the
    consumer that follows equals the pool's matrix. Over the seeds every
    (mutation, consumer) pair occurs, and every walk appends once by
    reallocation and once in place (test_lifecycle_host.py)."""
    import gdist
    p = LR.pool("dna")
    h, released = None, False
    for step, op in enumerate(LR.walk(seed, LR.STEPS)):
        kind, idx = op["op"], op["idx"]
        where = (seed, step, kind)
        if kind == "pack":
            if h is not None:
                h.free()
            h, released = pool_sets(ctx, idx, p), False
        elif kind == "append":
            assert h.append([p.seqs[i] for i in op["batch"]]) == len(idx) - len(op["batch"]), where
        elif kind == "append_empty":
            info = h.bitset_info()
            assert h.append([]) == len(idx), where
            assert h.bitset_info() == info, where                      # built bitsets are kept
        elif kind == "concat":
            other = pool_sets(ctx, op["other"], p)
            res = other.concat(h) if op["other_first"] else h.concat(other)
            h.free()
            other.free()
            h = res
        elif kind == "build":
            h.build_bitsets(keep_singletons=op["keep"], rare_threshold=op["T"])
            assert h.bitset_info()[0] >= 0, where
        elif kind == "prepare_auto":
            m, _, _ = h.prepare(gdist.METHOD_AUTO, op["pairs"])
            assert m in (gdist.METHOD_SORTED, gdist.METHOD_BITSET), where
        elif kind == "release":
            if h.bitset_info()[0] < 0:
                h.build_bitsets()                                      # the release needs bitsets to keep
            h.release_codes()
            released = True
        else:
            assert kind in LR.CONSUMERS and not (released and kind in LR.NEEDS_CODES), where
            try:
                apply_consumer(ctx, h, op, p)
            except AssertionError as e:
                raise AssertionError(f"walk {seed} step {step}: {op}") from e
            continue
        assert len(h) == len(idx), where
        assert np.array_equal(h.sizes(), p.sizes[idx]), where
        if not released:
            check_csr(h, *p.csr(idx), tag=where)
    h.free()
