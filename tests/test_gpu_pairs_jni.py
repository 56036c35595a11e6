"""nPairs of the JNI shim through the fake JVM (tests/jni_harness): the pair
list of MethodTableProcessor.java:258-276 in one native call, against the
oracle's matrices on the closest_ref recipe's mixed list."""
import ctypes as C

import numpy as np
import pytest

import closest_ref as CR
import pairs_ref as R

pytestmark = pytest.mark.gpu


def test_jni_pairs(tmp_path_factory):
    from jni_harness import harness
    from jni_harness.harness import INT, LONG, DOUBLE
    jvm = harness.FakeJVM(harness.current() or
                          harness.build(str(tmp_path_factory.mktemp("jni") / "libgdist_jni_test.so")))
    seqs = CR.recipe_sequences()
    eI, eD = R.recipe_matrices()
    rows, cols = R.recipe_lists()["mixed"]
    n = len(rows)
    xI, xD = R.pairs_ref(eI, eD, rows, cols)
    sig = [C.c_int64, C.c_int64, C.c_void_p, C.c_void_p, C.c_int32, C.c_int32, C.c_void_p, C.c_void_p]
    ctx = jvm.call_i("nCtxCreate", C.c_int64, [C.c_int32], 0)
    sets = jvm.call_i("nPack", C.c_int64, [C.c_int64, C.c_int32, C.c_int32, C.c_int32, C.c_void_p],
                      ctx, 0, 21, 0, jvm.byte_arrays(seqs))
    assert jvm.exception() is None and sets
    jr, jc = jvm.array(LONG, rows.tolist()), jvm.array(LONG, cols.tolist())
    for method in (1, 2, 0):
        ji, jd = jvm.array(INT, [7] * (n + 2)), jvm.array(DOUBLE, [7.5] * (n + 2))
        jvm.call_i("nPairs", None, sig, ctx, sets, jr, jc, method, 0, ji, jd)
        assert jvm.exception() is None
        assert jvm.read(ji, INT, n + 2) == xI.tolist() + [7, 7]
        got = np.array(jvm.read(jd, DOUBLE, n + 2))
        assert np.array_equal(got[:n].view(np.uint64), xD.view(np.uint64)) and np.all(got[n:] == 7.5)
    # one output alone
    jd = jvm.array(DOUBLE, [7.5] * n)
    jvm.call_i("nPairs", None, sig, ctx, sets, jr, jc, 0, 0, None, jd)
    assert jvm.exception() is None
    assert np.array_equal(np.array(jvm.read(jd, DOUBLE, n)).view(np.uint64), xD.view(np.uint64))
    ji = jvm.array(INT, [7] * n)
    jvm.call_i("nPairs", None, sig, ctx, sets, jr, jc, 0, 0, ji, None)
    assert jvm.exception() is None and jvm.read(ji, INT, n) == xI.tolist()
    # refusals: IllegalArgumentException, the arrays as they were
    ji, jd = jvm.array(INT, [7] * n), jvm.array(DOUBLE, [7.5] * n)
    jvm.call_i("nPairs", None, sig, ctx, sets, jr, jc, 0, 0, None, None)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "both outputs null")
    jvm.call_i("nPairs", None, sig, ctx, sets, jr, jvm.array(LONG, cols.tolist()[:-1]), 0, 0, ji, jd)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "rows and cols differ in length")
    jvm.call_i("nPairs", None, sig, ctx, sets, jr, jc, 0, 0, jvm.array(INT, [7] * (n - 1)), jd)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "I shorter than the pair list")
    jvm.call_i("nPairs", None, sig, ctx, sets, None, jc, 0, 0, ji, jd)
    assert jvm.exception() == ("java/lang/IllegalArgumentException", "null rows or cols")
    bad = rows.tolist()
    bad[5] = R.N
    jvm.call_i("nPairs", None, sig, ctx, sets, jvm.array(LONG, bad), jc, 0, 0, ji, jd)
    cls, msg = jvm.exception()
    assert cls == "java/lang/IllegalArgumentException" and "out of range" in msg
    jvm.call_i("nPairs", None, sig, ctx, 0, jr, jc, 0, 0, ji, jd)                       # a null collection
    assert jvm.exception()[0] == "java/lang/IllegalArgumentException"
    assert jvm.read(ji, INT, n) == [7] * n and jvm.read(jd, DOUBLE, n) == [7.5] * n
    jvm.call("nFree", None, sets)
    jvm.call("nCtxDestroy", None, ctx)
    assert jvm.exception() is None
    assert jvm.lib.fj_local_refs() == 0
