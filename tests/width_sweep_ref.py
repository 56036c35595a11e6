"""Expected answers of the sketch-error sweep (gdist_width_sweep), from the
oracle alone: no call into the library. Shared by test_width_sweep_host.py
(CPU) and test_gpu_width_sweep.py.

Per size s the sketches are the first s hashes of the signatures built at the
largest size (the prefix property: sorted distinct hashes, truncated), the
sketch distance of a pair is oracle.sketch_distance on the two prefixes at
width s, and the exact distance oracle.matrix's D. Over the pairs i < j whose
two distances differ: e = |r - s| * 2 / (r + s) in Python floats (fp64, one
rounding an operation), E = int(rint(ldexp(e, 62))), `sum` the Python-int sum
of E, total = float(sum) * 2**-62 (int -> float rounds to nearest even, the
scale is exact) and mean = total / pairs, pairs the number of pairs with
r < 1.0 (0.0 without any).
"""
import numpy as np

import oracle

TWO62 = 1 << 62


def pack(seqs, k, kind):
    """(off, codes, D) of the sequences: the oracle's sets and exact distances."""
    off, codes = oracle.pack(seqs, k, kind, 0)
    n = len(seqs)
    _, D = oracle.matrix(off, codes, 0, n, 0, n)
    return off, codes, D


def signatures(off, codes, k, kind, width):
    """The bottom-`width` signature of every set."""
    return [oracle.sketch(codes[off[i]:off[i + 1]], k, kind, width) for i in range(len(off) - 1)]


def sweep_ref(D, sigs, sizes, flags=0):
    """D: exact distances [n, n]; sigs: signatures of a width >= max(sizes).
    Returns (pairs, rows), rows a list of dicts with the fields of
    gdist_width_row (sum as a Python int)."""
    n = len(sigs)
    iu = [(i, j) for i in range(n) for j in range(i + 1, n)]
    pairs = sum(1 for i, j in iu if D[i, j] < 1.0)
    rows = []
    for s in sizes:
        pre = [np.ascontiguousarray(g[:s]) for g in sigs]
        differing, mx, tot = 0, 0.0, 0
        for i, j in iu:
            r = float(D[i, j])
            d = oracle.sketch_distance(pre[i], pre[j], s, flags)[0]
            if r != d:
                e = abs(r - d) * 2.0 / (r + d)
                differing += 1
                mx = e if e > mx else mx
                tot += int(np.rint(np.ldexp(e, 62)))
        total = float(tot) * 2.0 ** -62
        rows.append({"size": int(s), "dwarves": sum(1 for g in sigs if len(g) < s), "differing": differing,
                     "max_err": mx, "total": total, "mean": total / pairs if pairs else 0.0, "sum": tot})
    return pairs, rows


def expected(seqs, k, kind, sizes, flags=0, width=None):
    """(pairs, rows) of the sequences; width: of the collection the sweep
    reads (default max(sizes)): the answer does not depend on it."""
    off, codes, D = pack(seqs, k, kind)
    sigs = signatures(off, codes, k, kind, width or max(sizes))
    return sweep_ref(D, sigs, sizes, flags)
