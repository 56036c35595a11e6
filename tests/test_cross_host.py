"""CPU: the fixture of the cross-collection tests (cross_ref.py) holds every
condition those tests rely on, and the three gdist_cross_* entry points refuse
a null handle before any device work, with their message."""
import ctypes as C

import numpy as np

import cross_ref as X


def test_fixture_conditions():
    X.check_fixture()


def test_expected_matrices_are_the_oracle_slice():
    import closest_ref as R
    I, D = X.expected(0)
    full = R.recipe()[3]
    assert I.shape == D.shape == (X.NQ, X.NS)
    assert np.array_equal(D.view(np.uint64), full[np.ix_(X.QUERIES, X.SUBJECTS)].view(np.uint64))
    qn, sn = X.sizes()
    # a duplicate meets its subject with every code: d == 0 exactly there
    z = np.argwhere(D == 0.0)
    assert len(z) == 3 and all(I[a, b] == qn[a] == sn[b] for a, b in z)
    assert sorted(X.SUBJECTS[b] for _, b in z) == [5, 5, 77]


def test_null_handles_are_einval():
    from gdist import _lib as L
    I = np.full(4, -7, dtype=np.int32)
    D = np.full(4, 7.5, dtype=np.float64)
    rc = L.lib.gdist_cross_matrix(None, None, None, 0, 1, 0, 1, 0, L.ptr(I, C.c_int32), L.ptr(D, C.c_double), 1)
    assert rc == L.EINVAL and b"null context" in L.lib.gdist_last_error()
    idx = np.full(4, 99, dtype=np.int64)
    cnt = np.full(4, -9, dtype=np.int32)
    rc = L.lib.gdist_cross_closest(None, None, None, 0, 1, 0, 1, 0, 2, 0.9, L.ptr(idx, C.c_int64),
                                   L.ptr(D, C.c_double), L.ptr(cnt, C.c_int32))
    assert rc == L.EINVAL and b"null context" in L.lib.gdist_last_error()
    j, s, u = C.c_double(3.0), C.c_double(3.0), C.c_int64(3)
    rc = L.lib.gdist_ctx_cross_info(None, C.byref(j), C.byref(s), C.byref(u))
    assert rc == L.EINVAL and b"null context" in L.lib.gdist_last_error()
    # every output untouched
    assert np.all(I == -7) and np.all(D == 7.5) and np.all(idx == 99) and np.all(cnt == -9)
    assert (j.value, s.value, u.value) == (3.0, 3.0, 3)
