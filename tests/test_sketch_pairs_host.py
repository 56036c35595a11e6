"""Host side of the sketch pair list, without a device: the `minhash` method's
parameter parsing, header and registry entry (gdist/methods.py), the host
reduction SketchSets.row_query applies to a downloaded row of distances
(gdist.kmers.reduce_row_query) against the plain Python rules of
sketch_pairs_ref, and the unit cut of the shared pair-list plan
(csrc/pair_list.hpp: sketch chunks and the kmer cut by codes) in a stand-alone
program with its own main under AddressSanitizer + UBSan."""
import os
import shutil
import subprocess

import numpy as np
import pytest

import sketch_pairs_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NO_DEVICE = object()        # stands in for a Context: nothing here makes a device call


def make(parms=None):
    from gdist import methods as M
    m = M.DistanceMethod.create("minhash", NO_DEVICE)
    if parms is not None:
        m.parseParmString(parms)
    return m


def test_minhash_registry_and_defaults():
    from gdist import methods as M
    assert M.DistanceMethod._registry["minhash"] is M.MinHashMethod
    m = M.DistanceMethod.create("MinHash", NO_DEVICE)
    assert isinstance(m, M.MinHashMethod) and m.ctx is NO_DEVICE
    assert (m.k, m.width) == (21, 1000) and str(m) == "MINHASH_K21_W1000"
    m.parseParmString("")
    assert (m.k, m.width) == (21, 1000)
    assert m.pair_distances([]) == [] and m.getDistances(None, []) == [] and m.pair_calls == 0


@pytest.mark.parametrize("parms, k, w", [("K=15,W=64", 15, 64), ("W=64 K=15", 15, 64), ("k=8", 8, 1000),
                                         ("width=1", 21, 1), ("KMER=31, WIDTH=20000", 31, 20000)])
def test_minhash_parameters(parms, k, w):
    m = make(parms)
    assert (m.k, m.width) == (k, w) and str(m) == f"MINHASH_K{k}_W{w}"


@pytest.mark.parametrize("parms", ["K=x", "W=", "W=1.5", "K=1", "W=0", "W=-3", "S=5", "K", "21"])
def test_minhash_bad_parameters(parms):
    from gdist.processors import ParseFailureException
    with pytest.raises(ParseFailureException):
        make(parms)


def test_minhash_header_in_method_file():
    """read_method_file gives the column headers MethodTableProcessor writes."""
    import io

    from gdist import methods as M
    ms = M.read_method_file(io.StringIO("type\tparms\nkmer\tK=21\nminhash\tK=21,W=500\nminhash\n"), NO_DEVICE)
    assert [str(m) for m in ms] == ["KMER_K21", "MINHASH_K21_W500", "MINHASH_K21_W1000"]


NAN = float("nan")
ROWS = {
    "plain": [0.9, 0.25, 0.5, 1.0],
    "tie": [1.0, 0.0, 1.0, 0.0],
    "tie_first": [0.125, 0.125, 0.125],
    "all_ones": [1.0, 1.0, 1.0],
    "nan_first": [NAN, 0.75, NAN, 0.5],
    "only_nan": [NAN, NAN],
    "nan_and_ones": [NAN, 1.0],
    "one": [0.0],
    "empty": [],
}


@pytest.mark.parametrize("name", list(ROWS))
def test_reduce_row_query(name):
    from gdist import _lib as L
    from gdist.kmers import reduce_row_query
    ds = ROWS[name]
    got = reduce_row_query(np.array(ds, np.float64), L.QUERY_ALL)
    assert np.array_equal(R.bits(got), R.bits(ds))
    assert reduce_row_query(ds, L.QUERY_ARGMIN) == R.argmin(ds)
    for t in (0.0, 0.125, 0.5, 0.99, 1.0):
        hit = reduce_row_query(ds, L.QUERY_ANY_LE, t)
        assert hit is R.any_le(ds, t), t


def test_reduce_row_query_rules():
    """The rules themselves, spelt out (gdist_row_query in gdist.h)."""
    from gdist import _lib as L
    from gdist.kmers import reduce_row_query
    assert reduce_row_query(ROWS["tie"], L.QUERY_ARGMIN) == (1, 0.0)           # the lowest position
    assert reduce_row_query(ROWS["all_ones"], L.QUERY_ARGMIN) == (-1, 1.0)     # none below 1.0
    assert reduce_row_query(ROWS["all_ones"], L.QUERY_ANY_LE, 1.0) is True
    assert reduce_row_query(ROWS["nan_first"], L.QUERY_ARGMIN) == (3, 0.5)     # NaN never qualifies
    assert reduce_row_query(ROWS["only_nan"], L.QUERY_ARGMIN) == (-1, 1.0)
    assert reduce_row_query(ROWS["only_nan"], L.QUERY_ANY_LE, 1.0) is False
    with pytest.raises(ValueError):
        reduce_row_query(ROWS["plain"], 7)


def test_unit_count():
    assert R.unit_count([]) == 0
    assert R.unit_count([5] * 63) == R.unit_count([5] * 64) == 1 and R.unit_count([5] * 65) == 2
    assert R.unit_count([3] * 200 + [1, 2]) == 4 + 2
    rows, _ = R.runs_and_singles()
    assert R.unit_count(rows) == 38


def test_pair_list_plan_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "pair_list_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "pair_list_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]
