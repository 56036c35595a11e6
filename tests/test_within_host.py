"""CPU: the pairs-within-a-distance entry point (gdist_within) is declared,
exported and bound; it refuses a null context without touching the device or
its outputs; and the tests' reference answer (within_ref) is right on a
hand-made matrix."""
import ctypes as C
import os
import re

import numpy as np

import within_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


def test_within_is_declared_exported_and_bound():
    from gdist import _lib
    header = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "gdist.h")).read(), flags=re.S)
    m = re.search(r"\bint\s+gdist_within\s*\(([^;]*?)\)\s*;", header)
    assert m, "include/gdist.h does not declare gdist_within"
    assert len(m.group(1).split(",")) == 14
    t = re.search(r"\bint\s+gdist_ctx_within_timing\s*\(([^;]*?)\)\s*;", header)
    assert t and len(t.group(1).split(",")) == 3
    dll = C.CDLL(_lib.LIB_PATH)
    for name in ("gdist_within", "gdist_ctx_within_timing"):
        assert hasattr(dll, name)
        assert name in _lib.EXPORTED
    assert _lib.lib.gdist_abi_version() == 1


def test_within_null_context_is_einval():
    from gdist import _lib
    rowptr, cols, d = np.full(3, -7, np.int64), np.full(4, -7, np.int64), np.full(4, 7.5)
    total = C.c_int64(-7)
    _lib.lib.gdist_triangle_partition(-1, 4, 1, _lib.ptr(np.zeros(5, np.int64), C.c_int64))   # another message first
    rc = _lib.lib.gdist_within(None, None, 0, 2, 0, 2, _lib.METHOD_AUTO, 0, 0.9, 4, _lib.ptr(rowptr, C.c_int64),
                               _lib.ptr(cols, C.c_int64), _lib.ptr(d, C.c_double), C.byref(total))
    assert rc == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error()
    assert np.all(rowptr == -7) and np.all(cols == -7) and np.all(d == 7.5) and total.value == -7
    m, s = C.c_double(7.5), C.c_double(7.5)
    assert _lib.lib.gdist_ctx_within_timing(None, C.byref(m), C.byref(s)) == _lib.EINVAL
    assert b"null context" in _lib.lib.gdist_last_error() and (m.value, s.value) == (7.5, 7.5)


def test_within_ref_vs_brute_force():
    nan = float("nan")
    D = np.array([[0.0, 0.25, 0.25, 1.0, nan, 0.5],
                  [0.25, 0.0, 0.5, 0.25, 0.25, 1.0],
                  [0.25, 0.5, 0.0, 0.0, 1.0, 1.0],
                  [1.0, 0.25, 0.0, 0.0, 1.0, 1.0],
                  [nan, 0.25, 1.0, 1.0, nan, 1.0],
                  [0.5, 1.0, 1.0, 1.0, 1.0, 0.0]])
    regions = [((0, 6), (0, 6)), ((2, 4), (1, 5)), ((1, 6), (0, 3)), ((0, 2), (3, 6))]
    for (r0, r1), (c0, c1) in regions:
        for upper, keep_self in ((False, False), (False, True), (True, False), (True, True)):
            for md in (0.0, 0.25, 0.3, 0.99, 1.0):
                sub = D[r0:r1, c0:c1]
                rowptr, cols, d = R.within_ref(sub, md, r0, c0, upper, keep_self)
                assert rowptr.dtype == np.int64 and cols.dtype == np.int64 and d.dtype == np.float64
                assert rowptr[0] == 0 and rowptr[-1] == len(cols) == len(d)
                assert R.as_lists(rowptr, cols, d) == R.within_brute(sub, md, r0, c0, upper, keep_self), \
                    (r0, r1, c0, c1, upper, keep_self, md)
    # ties keep column order, NaN is never listed, 1.0 is listed only from max_dist 1.0 on
    rowptr, cols, d = R.within_ref(D, 1.0)
    assert rowptr.tolist() == [0, 4, 9, 14, 19, 23, 28]
    assert cols[:4].tolist() == [1, 2, 3, 5] and d[:4].tolist() == [0.25, 0.25, 1.0, 0.5]
    assert cols[19:23].tolist() == [1, 2, 3, 5]                     # row 4: its two NaN cells left out
    assert np.diff(R.within_ref(D, 0.99)[0]).tolist() == [3, 4, 3, 2, 1, 1]
    # the diagonal: only with keep_self, and row 4's own cell is NaN even then
    assert np.diff(R.within_ref(D, 0.0)[0]).tolist() == [0, 0, 1, 1, 0, 0]
    assert np.diff(R.within_ref(D, 0.0, keep_self=True)[0]).tolist() == [1, 1, 2, 2, 0, 1]
    # upper: the pairs j > i of the full answer, whatever keep_self says
    rowptr, cols, d = R.within_ref(D, 0.3, upper=True, keep_self=True)
    assert R.as_lists(rowptr, cols, d) == [[(1, 0.25), (2, 0.25)], [(3, 0.25), (4, 0.25)], [(3, 0.0)], [], [], []]
    # a rectangle: rows 2..3 against columns 1..4, global indices, self excluded by global index
    rowptr, cols, d = R.within_ref(D[2:4, 1:5], 1.0, r0=2, c0=1)
    assert rowptr.tolist() == [0, 3, 6] and cols.tolist() == [1, 3, 4, 1, 2, 4]
    assert d.tolist() == [0.5, 0.0, 1.0, 0.25, 0.0, 1.0]
    # a negative threshold lists nothing, +inf everything but NaN and the diagonal
    assert R.within_ref(D, -1.0)[0].tolist() == [0] * 7
    assert int(R.within_ref(D, float("inf"))[0][-1]) == 36 - 6 - 2
