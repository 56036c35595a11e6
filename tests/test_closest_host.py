"""CPU: the exact nearest-neighbour entry point (gdist_closest) is declared,
exported and bound; it refuses a null context without touching the device;
and the tests' reference answer (closest_ref) is right on a hand-made matrix."""
import ctypes as C
import os
import re

import numpy as np

import closest_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_closest_is_declared_exported_and_bound():
    from gdist import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdist.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gdist_closest\s*\(([^;]*?)\)\s*;", header)
    assert m, "include/gdist.h does not declare gdist_closest"
    assert len(m.group(1).split(",")) == 13
    assert re.search(r"#define\s+GDIST_CLOSEST_KEEP_SELF\s+0x1000u", header)
    assert re.search(r"#define\s+GDIST_CLOSEST_MAX_N\s+512\b", header)
    assert hasattr(C.CDLL(_lib.LIB_PATH), "gdist_closest")
    assert "gdist_closest" in _lib.EXPORTED
    assert (_lib.CLOSEST_KEEP_SELF, _lib.CLOSEST_MAX_N) == (0x1000, 512)
    assert _lib.lib.gdist_abi_version() == 1


def test_closest_null_context_is_einval():
    from gdist import _lib
    idx, d, cnt = np.zeros(4, np.int64), np.zeros(4, np.float64), np.zeros(2, np.int32)
    _lib.lib.gdist_triangle_partition(-1, 4, 1, _lib.ptr(np.zeros(5, np.int64), C.c_int64))   # another message first
    rc = _lib.lib.gdist_closest(None, None, 0, 2, 0, 2, _lib.METHOD_AUTO, 0, 2, 0.9, _lib.ptr(idx, C.c_int64),
                                _lib.ptr(d, C.c_double), _lib.ptr(cnt, C.c_int32))
    assert rc == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error()
    assert not idx.any() and not d.any() and not cnt.any()


def test_closest_ref_vs_brute_force():
    nan = float("nan")
    D = np.array([[0.0, 0.25, 0.25, 1.0, nan, 0.5],
                  [0.25, 0.0, 0.5, 0.25, 0.25, 1.0],
                  [0.25, 0.5, 0.0, 0.0, 1.0, 1.0],
                  [1.0, 0.25, 0.0, 0.0, 1.0, 1.0],
                  [nan, 0.25, 1.0, 1.0, nan, 1.0],
                  [0.5, 1.0, 1.0, 1.0, 1.0, 0.0]])
    for keep_self in (False, True):
        for n in (1, 2, 3, 6, 8):
            for md in (0.0, 0.25, 0.3, 0.99, 1.0):
                idx, d, cnt = R.closest_ref(D, n, md, keep_self=keep_self)
                assert R.as_lists(idx, d, cnt) == R.closest_brute(D, n, md, keep_self=keep_self), (keep_self, n, md)
                for a in range(6):
                    assert np.all(idx[a, cnt[a]:] == -1) and np.all(d[a, cnt[a]:] == 1.0)
    # ties broken by column, NaN never listed, 1.0 listed only from max_dist 1.0 on
    idx, d, cnt = R.closest_ref(D, 6, 1.0)
    assert idx[0].tolist() == [1, 2, 5, 3, -1, -1] and cnt[0] == 4
    assert idx[4].tolist() == [1, 2, 3, 5, -1, -1]
    assert R.closest_ref(D, 6, 0.99)[2].tolist() == [3, 4, 3, 2, 1, 1]
    # a rectangle: rows 2..3 against columns 1..4, global indices, self excluded by global index
    idx, d, cnt = R.closest_ref(D[2:4, 1:5], 3, 1.0, r0=2, c0=1)
    assert idx.tolist() == [[3, 1, 4], [2, 1, 4]] and d.tolist() == [[0.0, 0.5, 1.0], [0.0, 0.25, 1.0]]
    assert R.as_lists(idx, d, cnt) == R.closest_brute(D[2:4, 1:5], 3, 1.0, r0=2, c0=1)
