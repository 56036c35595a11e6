"""The triple records of the sparse tile kernel's 3 x 3 walk on the host:
tests/sparse_triple_check.cpp packs and unpacks them with the functions the
record build and the walk call (csrc/sparse_triple.hpp), under the
sanitizers, and the binding exports the query the GPU test reads them by."""
import ctypes as C
import os
import shutil
import subprocess

import pytest

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_triple_records_under_sanitizers(tmp_path):
    cxx = shutil.which("c++") or shutil.which("g++") or shutil.which("clang++")
    if cxx is None:
        pytest.fail("no host C++ compiler on PATH")
    exe = str(tmp_path / "sparse_triple_check")
    subprocess.run([cxx, "-std=c++17", "-O1", "-g", "-Wall", "-Werror", "-fsanitize=address,undefined",
                    "-fno-sanitize-recover=all", "-I", os.path.join(ROOT, "genome.distance_amd", "csrc"),
                    os.path.join(ROOT, "tests", "sparse_triple_check.cpp"), "-o", exe], check=True)
    r = subprocess.run([exe], capture_output=True, text=True)
    assert r.returncode == 0, r.stdout[-4000:] + r.stderr[-4000:]
    assert " 0 failures" in r.stdout, r.stdout[-2000:]


def test_sparse_triples_is_exported():
    from gdist import _lib
    assert "gdist_sets_sparse_triples" in _lib.EXPORTED
    assert hasattr(C.CDLL(_lib.LIB_PATH), "gdist_sets_sparse_triples")
    out = (C.c_int64 * 5)(*([-7] * 5))
    assert _lib.lib.gdist_sets_sparse_triples(None, out) == _lib.EINVAL      # a null collection
    assert list(out) == [-7] * 5
