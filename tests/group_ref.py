"""Expected answers of the in-group / out-group distance summary
(gdist_group_stats), from a distance matrix and labels alone: numpy masks,
Python ints and fractions.Fraction, no call into the library. Shared by
test_group_host.py (CPU) and test_gpu_group_stats.py.

A pair is classified as GroupTypeSpec.java:77-95 classifies it: a label < 0 on
either set is a bad pair and nothing else; equal labels are in-group, others
out-group; within a side d == 1.0 is counted in `ones`, NaN in `nans`, any
other d is summarised. Every summarised d must be an integer multiple of
2^-53 (asserted): m = d * 2^53, and sum / sumsq are the exact integers
sum m / sum m * m. mean and var are exact Fractions (var bias-corrected,
None below two values).
"""
import math
from fractions import Fraction

import numpy as np

TWO53 = 1 << 53


def exact_m(values):
    """m = d * 2^53 of every d as Python ints; asserts each is an integer."""
    out = []
    for d in values:
        p, q = float(d).as_integer_ratio()
        assert 0 <= p < q and TWO53 % q == 0, f"{d!r} is not a multiple of 2^-53 in [0, 1)"
        out.append(p * (TWO53 // q))
    return out


def side_ref(values):
    """One side from the distances that fell into it (any order)."""
    v = np.asarray(values, dtype=np.float64).ravel()
    isnan = np.isnan(v)
    one = v == 1.0
    num = v[~isnan & ~one]
    m = exact_m(num.tolist())
    n = len(m)
    s, q = sum(m), sum(x * x for x in m)
    side = {"n": n, "ones": int(one.sum()), "nans": int(isnan.sum()), "sum": s, "sumsq": q,
            "min": float(num.min()) if n else 1.0, "max": float(num.max()) if n else 1.0,
            "mean": Fraction(s, n * TWO53) if n else None,
            "var": Fraction(n * q - s * s, n * (n - 1) * TWO53 * TWO53) if n > 1 else None}
    return side


def group_ref(D, labels, r0=0, c0=0, upper=True):
    """D[a, b] = d(set r0 + a, set c0 + b); labels [T, N] (or [N]) over the whole
    collection. upper: only the pairs with global column > global row. Returns
    one dict per grouping: {"bad": int, "sides": [in, out]} (side_ref dicts)."""
    D = np.asarray(D, dtype=np.float64)
    labels = np.atleast_2d(np.asarray(labels, dtype=np.int64))
    nr, nc = D.shape
    rows, cols = np.arange(nr) + r0, np.arange(nc) + c0
    take = cols[None, :] > rows[:, None] if upper else np.ones((nr, nc), dtype=bool)
    out = []
    for lab in labels:
        la, lb = lab[rows][:, None], lab[cols][None, :]
        isbad = take & ((la < 0) | (lb < 0))
        ok = take & ~isbad
        same = ok & (la == lb)
        out.append({"bad": int(isbad.sum()), "sides": [side_ref(D[same]), side_ref(D[ok & ~same])]})
    return out


def mean_within(x, exact, ulps):
    """|x - exact| <= ulps * ulp(x), exactly."""
    return abs(Fraction(x) - exact) <= ulps * Fraction(math.ulp(x))


def sdev_within(x, var, ulps):
    """|x - sqrt(var)| <= ulps * ulp(x), exactly (by the squares)."""
    u = ulps * Fraction(math.ulp(x))
    lo, hi = Fraction(x) - u, Fraction(x) + u
    return (lo <= 0 or lo * lo <= var) and var <= hi * hi


def check_side(got, exp, where=""):
    """A gdist_group_side-like object (attributes n, ones, nans, min, max, mean,
    sdev and the limb arrays sum / sumsq) against a side_ref dict: integers and
    the bits of min / max with ==, mean within 1 ulp, sdev within 2 ulp."""
    limbs = lambda v: sum(int(x) << (64 * i) for i, x in enumerate(v))
    bits = lambda x: np.float64(x).view(np.uint64)
    assert (got.n, got.ones, got.nans) == (exp["n"], exp["ones"], exp["nans"]), where
    assert limbs(got.sum) == exp["sum"] and limbs(got.sumsq) == exp["sumsq"], where
    assert bits(got.min) == bits(exp["min"]) and bits(got.max) == bits(exp["max"]), where
    if exp["n"] == 0:
        assert (got.min, got.max, got.mean, got.sdev) == (1.0, 1.0, 1.0, 0.0), where
        return
    assert mean_within(got.mean, exp["mean"], 1), (where, got.mean, float(exp["mean"]))
    if exp["n"] == 1:
        assert got.sdev == 0.0 and bits(got.sdev) == 0, where
    else:
        assert sdev_within(got.sdev, exp["var"], 2), (where, got.sdev, float(exp["var"]) ** 0.5)


def check_stats(sides, bad, ref, where=""):
    """The [2 T] side array and [T] bad counts of a call against group_ref's answer."""
    assert len(bad) == len(ref) and len(sides) == 2 * len(ref)
    for t, r in enumerate(ref):
        assert int(bad[t]) == r["bad"], (where, t)
        for k in range(2):
            check_side(sides[2 * t + k], r["sides"][k], f"{where} type {t} side {k}")
