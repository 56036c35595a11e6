"""CPU: the host side of the in-group / out-group distance summary.

gdist_group_stats_merge (host only, exact) through ctypes on hand-made
structs; the arithmetic header csrc/group_stats_host.hpp as a stand-alone
program under AddressSanitizer + UBSan; GroupStats.merge and the distCheck
table of processors.write_distance_check on group_ref's answers; and
group_ref itself on a hand-made matrix. No device call is made."""
import ctypes as C
import io
import os
import re
import shutil
import subprocess
from fractions import Fraction

import numpy as np
import pytest

import group_ref as G

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
ALL = (1 << 64) - 1
NAN = float("nan")

# 6 sets: d(i, j) symmetric, multiples of 2^-53, with 1.0, NaN and exact zeros
D6 = np.array([[0.0, 0.25, 0.5, 1.0, NAN, 0.75],
               [0.25, 0.0, 1.0 - 2.0 ** -53, 0.125, 1.0, 1.0],
               [0.5, 1.0 - 2.0 ** -53, 0.0, 0.0, 1.0, 2.0 ** -53],
               [1.0, 0.125, 0.0, 0.0, 0.375, 1.0],
               [NAN, 1.0, 1.0, 0.375, NAN, 0.625],
               [0.75, 1.0, 2.0 ** -53, 1.0, 0.625, 0.0]])
LAB6 = np.array([[0, 0, 0, 1, 1, 1],
                 [0, 0, 0, 0, 0, 0],
                 [0, 1, 2, 3, 4, 5],
                 [-1, 0, 1, 0, -1, 1]], dtype=np.int32)


def limbs_of(v, n):
    return [(v >> (64 * i)) & ALL for i in range(n)]


def make_side(L, ref, mean=-7.0, sdev=-7.0):
    """A gdist_group_side from a side_ref dict; mean / sdev as given (garbage
    by default: a merge must recompute them)."""
    s = L.GroupSide()
    s.n, s.ones, s.nans = ref["n"], ref["ones"], ref["nans"]
    s.min, s.max, s.mean, s.sdev = ref["min"], ref["max"], mean, sdev
    for i, x in enumerate(limbs_of(ref["sum"], 2)):
        s.sum[i] = x
    for i, x in enumerate(limbs_of(ref["sumsq"], 3)):
        s.sumsq[i] = x
    return s


def stats_of(ref):
    """A GroupStats holding group_ref's answer: the integer fields from the
    reference, mean and sdev by merging into the empty summary."""
    import gdist
    from gdist import _lib as L
    T = len(ref)
    sides, bad = (L.GroupSide * (2 * T))(), (C.c_int64 * T)()
    for t, r in enumerate(ref):
        bad[t] = r["bad"]
        for k in range(2):
            sides[2 * t + k] = make_side(L, r["sides"][k])
    return gdist.GroupStats.empty(T).merge(gdist.GroupStats(sides, bad))


def merge1(L, a, b):
    """acc = a; acc += b for one grouping whose in side is a / b (out side empty)."""
    acc, part = (L.GroupSide * 2)(), (L.GroupSide * 2)()
    acc[0], part[0] = a, b
    for arr in (acc, part):
        arr[1].min = arr[1].max = arr[1].mean = 1.0
    ba, bp = (C.c_int64 * 1)(3), (C.c_int64 * 1)(4)
    assert L.lib.gdist_group_stats_merge(C.addressof(acc), ba, C.addressof(part), bp, 1) == 0
    assert ba[0] == 7
    return acc[0]


def test_group_stats_is_declared_exported_and_bound():
    from gdist import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdist.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gdist_group_stats\s*\(([^;]*?)\)\s*;", header)
    assert m and len(m.group(1).split(",")) == 12
    assert re.search(r"#define\s+GDIST_GROUP_MAX_TYPES\s+8\b", header)
    lib = C.CDLL(_lib.LIB_PATH)
    for name in ("gdist_group_stats", "gdist_group_stats_merge", "gdist_ctx_group_stats_timing"):
        assert hasattr(lib, name) and name in _lib.EXPORTED
    assert C.sizeof(_lib.GroupSide) == 96 and _lib.GROUP_MAX_TYPES == 8
    assert _lib.lib.gdist_abi_version() == 1


def test_group_ref_on_a_hand_made_matrix():
    ref = G.group_ref(D6, LAB6, upper=True)
    blk, one, solo, holes = ref
    # grouping {0,1,2} {3,4,5}, upper: in = (0,1) (0,2) (1,2) (3,4) (3,5) (4,5)
    s = blk["sides"][0]
    assert (s["n"], s["ones"], s["nans"], blk["bad"]) == (5, 1, 0, 0)
    assert s["sum"] == sum(int(Fraction(x) * G.TWO53) for x in (0.25, 0.5, 1.0 - 2.0 ** -53, 0.375, 0.625))
    assert (s["min"], s["max"]) == (0.25, 1.0 - 2.0 ** -53)
    o = blk["sides"][1]
    assert (o["n"], o["ones"], o["nans"]) == (4, 4, 1) and (o["min"], o["max"]) == (0.0, 0.75)
    assert one["sides"][1]["n"] == 0 and one["sides"][1]["mean"] is None and one["sides"][0]["n"] == 9
    assert solo["sides"][0]["n"] == 0 and solo["sides"][1] == one["sides"][0]
    assert holes["bad"] == 9 and sum(holes["sides"][k][f] for k in range(2) for f in ("n", "ones", "nans")) == 6
    # the full region counts both orders and the diagonal: set 4 is NaN from itself
    full = G.group_ref(D6, LAB6, upper=False)
    assert full[2]["sides"][0]["n"] == 5 and full[2]["sides"][0]["nans"] == 1 and full[2]["sides"][0]["max"] == 0.0
    assert full[1]["sides"][0]["n"] == 2 * 9 + 5 and full[3]["bad"] == 20
    # a rectangle addresses the labels by global index
    rect = G.group_ref(D6[1:3, 2:6], LAB6, r0=1, c0=2, upper=True)
    assert rect[0]["sides"][0]["n"] == 1 and rect[0]["sides"][1]["n"] == 3 and rect[0]["sides"][1]["ones"] == 3
    with pytest.raises(AssertionError):
        G.side_ref([0.25 + 2.0 ** -54])             # a double, but not a multiple of 2^-53
    assert G.mean_within(0.1, Fraction(0.1) + Fraction(1, 1 << 56), 1)
    assert not G.mean_within(0.5, Fraction(0.5) + Fraction(3, 1 << 53), 1)
    assert G.sdev_within(2.0 ** 0.5, Fraction(2), 1) and not G.sdev_within(1.5, Fraction(2), 2)


def test_merge_carries_and_placeholders():
    from gdist import _lib as L
    # carries out of sum[0], sumsq[0] and sumsq[1]
    a = {"n": 3, "ones": 4, "nans": 0, "min": 0.125, "max": 0.5, "sum": ALL, "sumsq": (1 << 128) - 1}
    b = {"n": 2, "ones": 5, "nans": 1, "min": 0.0625, "max": 0.25, "sum": 1, "sumsq": 1}
    r = merge1(L, make_side(L, a), make_side(L, b))
    assert (r.n, r.ones, r.nans, r.min, r.max) == (5, 9, 1, 0.0625, 0.5)
    assert list(r.sum) == [0, 1] and list(r.sumsq) == [0, 0, 1]
    # an n == 0 side merged from either position, and with itself
    ref = G.group_ref(D6, LAB6, upper=True)
    full_side, empty_side = ref[1]["sides"]
    assert full_side["n"] == 9 and empty_side["n"] == 0
    want = merge1(L, make_side(L, empty_side, 1.0, 0.0), make_side(L, full_side))
    G.check_side(want, full_side)
    for x, y in ((full_side, empty_side), (empty_side, full_side)):
        got = merge1(L, make_side(L, x), make_side(L, y))
        assert bytes(got) == bytes(want)
    e = merge1(L, make_side(L, empty_side), make_side(L, empty_side))
    assert (e.n, e.min, e.max, e.mean, e.sdev) == (0, 1.0, 1.0, 1.0, 0.0) and not any(e.sum) and not any(e.sumsq)
    # n == 1: sdev 0.0, mean the value
    solo = G.side_ref([0.375])
    r = merge1(L, make_side(L, empty_side), make_side(L, solo))
    assert (r.n, r.mean, r.sdev, r.min, r.max) == (1, 0.375, 0.0, 0.375, 0.375)
    # 1 + 1 = 2 values: mean 0.5, variance 0.125
    r = merge1(L, make_side(L, G.side_ref([0.25])), make_side(L, G.side_ref([0.75])))
    G.check_side(r, G.side_ref([0.75, 0.25]))
    assert r.mean == 0.5 and r.sdev == 0.125 ** 0.5


def test_merge_mean_and_sdev_against_fractions():
    """mean within 1 ulp and sdev within 2 ulp of the exact values, on random
    multiples of 2^-53 of every magnitude and on sums past 64 and 128 bits."""
    from gdist import _lib as L
    rng = np.random.default_rng(7)
    empty = G.side_ref([])
    cases = []
    for n in (2, 3, 17, 1000):
        num = rng.integers(1, 1 << 40, size=n)
        den = num + rng.integers(0, 1 << 40, size=n)
        cases.append(1.0 - num / den)                      # the library's form: 1 - fl(a / b)
        cases.append(rng.integers(0, 1 << 20, size=n) * 2.0 ** -53)   # a few units of 2^-53
        cases.append(0.5 + rng.integers(0, 1 << 10, size=n) * 2.0 ** -53)   # cancellation in n Q - S^2
    cases.append(np.full(5000, 1.0 - 2.0 ** -53))          # sum past 64 bits, equal values: variance 0
    cases.append(np.concatenate([np.full(3000, 1.0 - 2.0 ** -53), np.zeros(3000)]))
    for v in cases:
        v = v[v < 1.0]
        ref = G.side_ref(v)
        half = len(v) // 2
        got = merge1(L, make_side(L, G.side_ref(v[:half])), make_side(L, G.side_ref(v[half:])))
        G.check_side(got, ref)
        assert bytes(got) == bytes(merge1(L, make_side(L, empty), make_side(L, ref)))
    assert G.side_ref(cases[-2])["sum"] >> 64 and G.side_ref(cases[-1])["var"] > 0
    assert merge1(L, make_side(L, empty), make_side(L, G.side_ref(cases[-2]))).sdev == 0.0
    # a third limb of sumsq: 2^24 values of 2/3-ish as one hand-made struct
    m = int(Fraction(1.0 - 1.0 / 3.0) * G.TWO53)
    n = 1 << 24
    big = {"n": n, "ones": 0, "nans": 0, "min": 0.0, "max": 1.0 - 1.0 / 3.0, "sum": (n - 4096) * m,
           "sumsq": (n - 4096) * m * m}
    big["mean"] = Fraction(big["sum"], n * G.TWO53)
    big["var"] = Fraction(n * big["sumsq"] - big["sum"] ** 2, n * (n - 1) * G.TWO53 ** 2)
    assert big["sumsq"] >> 128
    G.check_side(merge1(L, make_side(L, empty), make_side(L, big)), big)


def test_merge_refuses_bad_arguments():
    from gdist import _lib as L
    acc, part = (L.GroupSide * 2)(), (L.GroupSide * 2)()
    b = (C.c_int64 * 1)()
    before = bytes(acc)
    assert L.lib.gdist_group_stats_merge(None, b, C.addressof(part), b, 1) == L.EINVAL
    assert L.lib.gdist_group_stats_merge(C.addressof(acc), b, None, b, 1) == L.EINVAL
    assert L.lib.gdist_group_stats_merge(C.addressof(acc), None, C.addressof(part), b, 1) == L.EINVAL
    assert L.lib.gdist_group_stats_merge(C.addressof(acc), b, C.addressof(part), b, 0) == L.EINVAL
    assert L.lib.gdist_group_stats_merge(C.addressof(acc), b, C.addressof(part), b, 9) == L.EINVAL
    assert bytes(acc) == before
    # a null context is refused before anything is read or written
    lab = np.zeros(4, dtype=np.int32)
    assert L.lib.gdist_group_stats(None, None, 0, 2, 0, 2, 0, 0, 1, L.ptr(lab, C.c_int32), C.addressof(acc),
                                   b) == L.EINVAL
    assert b"null context" in L.lib.gdist_last_error() and bytes(acc) == before
    assert L.lib.gdist_ctx_group_stats_timing(None, None, None) == L.EINVAL


def test_host_arithmetic_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "group_stats_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "group_stats_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def test_group_stats_merge_in_python():
    import gdist
    top, bottom = G.group_ref(D6[:3], LAB6, r0=0, upper=True), G.group_ref(D6[3:], LAB6, r0=3, upper=True)
    whole = G.group_ref(D6, LAB6, upper=True)
    a, b, w = stats_of(top), stats_of(bottom), stats_of(whole)
    m = a.merge(b)
    assert m.tobytes() == w.tobytes() and b.merge(a).tobytes() == w.tobytes()
    assert m.tobytes() != a.tobytes() and a.tobytes() == stats_of(top).tobytes()      # merge returns a new object
    G.check_stats(m.sides, m.bad_raw, whole)
    assert m.n.shape == (4, 2) and m.n.dtype == np.int64 and m.mean.dtype == np.float64 and m.bad.shape == (4,)
    assert m.n[0].tolist() == [5, 4] and m.ones[0].tolist() == [1, 4] and m.nans[0].tolist() == [0, 1]
    assert m.bad.tolist() == [0, 0, 0, 9]
    assert m.sum[0][0] == whole[0]["sides"][0]["sum"] and m.sumsq[0][1] == whole[0]["sides"][1]["sumsq"]
    assert isinstance(m.sum[0][0], int)
    assert np.array_equal(m.low, m.mean - m.sdev) and np.array_equal(m.high, m.mean + m.sdev)
    back = gdist.GroupStats.frombytes(w.tobytes())
    assert back.tobytes() == w.tobytes() and back.sum == w.sum and np.array_equal(back.bad, w.bad)
    with pytest.raises(ValueError):
        gdist.GroupStats.frombytes(w.tobytes()[:-1])
    e = gdist.GroupStats.empty(4)
    assert e.merge(w).tobytes() == w.tobytes() and e.merge(e).tobytes() == e.tobytes()
    with pytest.raises(ValueError):
        a.merge(gdist.GroupStats.empty(3))


def expected_table(ref, names, name, header=True):
    """The distCheck text from group_ref's answer alone (Fractions rounded to
    the nearest double are what the library's 1 / 2 ulp bounds allow to differ;
    the hand-made cases below are exact in fp64)."""
    from gdist import java_double
    lines = ["dist_file\tgroup_type\tin_out\tmin\tlow\tmean\thigh\tmax\tones"] if header else []
    for r, gtype in zip(ref, names):
        for side, s in zip(("in", "out"), r["sides"]):
            if s["n"] == 0:
                vals = [1.0] * 5
            else:
                mean = float(s["mean"])
                sd = float(s["var"]) ** 0.5 if s["var"] is not None else 0.0
                vals = [s["min"], mean - sd, mean, mean + sd, s["max"]]
            lines.append("\t".join([name, gtype, side] + [java_double(v) for v in vals] + [str(s["ones"])]))
    return "\n".join(lines) + "\n"


def test_distance_check_formatting():
    from gdist import java_double, processors
    # values whose mean and sd are exact in fp64: 0.25 / 0.75 in, 0.5 alone out
    D = np.array([[0.0, 0.25, 0.5, 1.0], [0.25, 0.0, 0.75, 1.0], [0.5, 0.75, 0.0, 1.0], [1.0, 1.0, 1.0, 0.0]])
    ids = ["g1", "g2", "g3", "g4"]
    groupings = {"genus": {"g1": "A", "g2": "A", "g3": "B", "g4": "B"},
                 "species": {"g2": "x", "g3": "x", "g4": "y"},
                 "all": dict.fromkeys(ids, "same")}
    names, lab = processors.group_labels(ids, groupings)
    assert names == ["genus", "species", "all"]
    assert lab.dtype == np.int32 and lab.tolist() == [[0, 0, 1, 1], [-1, 0, 0, 1], [0, 0, 0, 0]]
    ref = G.group_ref(D, lab, upper=True)
    out = io.StringIO()
    assert processors.write_distance_check(stats_of(ref), names, out, "dists.tbl") == 3
    text = out.getvalue()
    assert text == expected_table(ref, names, "dists.tbl")
    rows = text.splitlines()
    assert rows[0] == "dist_file\tgroup_type\tin_out\tmin\tlow\tmean\thigh\tmax\tones"
    assert rows[1] == "dists.tbl\tgenus\tin\t0.25\t0.25\t0.25\t0.25\t0.25\t1"         # n == 1: sd 0.0
    sd = 0.03125 ** 0.5                                                              # of 0.5 and 0.75, exact
    assert rows[2] == f"dists.tbl\tgenus\tout\t0.5\t{java_double(0.625 - sd)}\t0.625\t{java_double(0.625 + sd)}\t0.75\t2"
    assert java_double(0.625 + sd) == "0.8017766952966369"
    assert rows[4] == "dists.tbl\tspecies\tout\t1.0\t1.0\t1.0\t1.0\t1.0\t2"          # nothing below 1.0
    assert rows[6] == "dists.tbl\tall\tout\t1.0\t1.0\t1.0\t1.0\t1.0\t0"              # no pair at all
    out = io.StringIO()
    processors.write_distance_check(stats_of(ref), names, out, "x", header=False)
    assert out.getvalue() == expected_table(ref, names, "x", header=False)
