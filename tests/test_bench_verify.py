"""bench.py's end-of-run verification: the independent numpy kmer recount
agrees with the oracle's packer, and verify_sample flags a wrong device
entry (CPU only: device buffers are faked)."""
import os
import sys

import numpy as np

import oracle

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
sys.path.insert(0, ROOT)
import bench  # noqa: E402
from gdist import synth  # noqa: E402


def test_recount_matches_oracle_pack():
    for protein, k, kind in ((False, 21, 0), (True, 8, 1)):
        g = [bytes(r) for r in synth.genomes(4, 4000, 0.05, 7, protein=protein)]
        off, codes = oracle.pack(g, k, kind, 0)
        for i in range(len(g)):
            mine = bench._kmer_codes(g[i], k, protein)
            assert np.array_equal(mine, np.asarray(codes[off[i]:off[i + 1]], dtype=np.uint64))


class _FakeBuf:
    def __init__(self, arr):
        self.arr = arr

    def to_host(self, dtype, count=None, offset=0):
        return self.arr.view(dtype)[offset:offset + count].copy()

    def from_host(self, a, offset=0):
        self.arr[offset:offset + len(a)] = a


def test_verify_sample_detects_mismatch():
    cfg = dict(length=3000, p_max=0.01, cfg=2, k=21, protein=False)
    n = 6
    g = [bytes(r) for r in synth.genomes(n, cfg["length"], cfg["p_max"], cfg["cfg"])]
    off, codes = oracle.pack(g, 21, 0, 0)
    eI, eD = oracle.matrix(off, codes, 0, n, 0, n)
    ident = lambda v: v   # noqa: E731  (single rank: max over ranks is the value)
    r0, r1 = 2, 5
    I = np.ascontiguousarray(eI[r0:r1].astype(np.int32)).ravel()
    D = np.ascontiguousarray(eD[r0:r1]).ravel()
    good = bench.verify_sample(cfg, "bitset", n, r0, r1, _FakeBuf(I), _FakeBuf(D), ident)
    assert good["ok"] and good["pairs_per_rank"] == 4
    bad_I = I.copy()
    bad_I[(2 - r0) * n + 3] += 1          # pair (2, 3) is the first one checked
    bad = bench.verify_sample(cfg, "bitset", n, r0, r1, _FakeBuf(bad_I), _FakeBuf(D), ident)
    assert not bad["ok"]
    assert bench.verify_sample(cfg, "sketch", n, r0, r1, None, None, ident) is None


def test_dump_outputs_writes_the_upper_triangle(tmp_path, monkeypatch):
    """--dump-outputs: the rows' I and D as float64, the entries the step
    leaves untouched (column <= row) as 0 whatever the buffers held there;
    past the byte limit the same seeded sample of rows and columns each time."""
    n, r0, r1 = 7, 2, 6
    rng = np.random.default_rng(1)
    I = rng.integers(1, 1000, (r1 - r0, n)).astype(np.int32)
    D = rng.random((r1 - r0, n))
    bI, bD = _FakeBuf(I.ravel().copy()), _FakeBuf(D.ravel().copy())
    info = bench.dump_outputs(str(tmp_path / "a"), bI, bD, n, r0, r1)
    gI, gD = np.load(tmp_path / "a" / "I.npy"), np.load(tmp_path / "a" / "D.npy")
    assert info["arrays"] == ["I.npy", "D.npy"] and info["rows"] == r1 - r0 and info["cols"] == n
    assert gI.dtype == np.float64 and gD.dtype == np.float64 and gI.shape == gD.shape == (r1 - r0, n)
    for i in range(r0, r1):
        for j in range(n):
            assert gI[i - r0, j] == (I[i - r0, j] if j > i else 0)
            assert gD[i - r0, j] == (D[i - r0, j] if j > i else 0.0)
    # a limit of 2 rows x 7 columns: a sample of the rows, whole
    monkeypatch.setattr(bench, "DUMP_BYTES", 2 * n * 16)
    one = bench.dump_outputs(str(tmp_path / "b"), bI, bD, n, r0, r1)
    two = bench.dump_outputs(str(tmp_path / "c"), bI, bD, n, r0, r1)
    assert one["rows"] == 2 and one["cols"] == n and one["of_rows"] == r1 - r0
    sI, sD = np.load(tmp_path / "b" / "I.npy"), np.load(tmp_path / "b" / "D.npy")
    assert sI.shape == (2, n) and sI.nbytes + sD.nbytes <= bench.DUMP_BYTES
    assert np.array_equal(sI, np.load(tmp_path / "c" / "I.npy")) and two["rows"] == 2
    assert all(any(np.array_equal(row, g) for g in gI) for row in sI)
    # a limit below one row: one row, a sample of its columns
    monkeypatch.setattr(bench, "DUMP_BYTES", 3 * 16)
    cut = bench.dump_outputs(str(tmp_path / "d"), bI, bD, n, r0, r1)
    assert cut["rows"] == 1 and cut["cols"] == 3 and np.load(tmp_path / "d" / "D.npy").shape == (1, 3)
    # several ranks share the limit and name their files
    monkeypatch.setattr(bench, "DUMP_BYTES", 64 << 20)
    r = bench.dump_outputs(str(tmp_path / "e"), bI, bD, n, r0, r1, rank=1, world=2)
    assert r["arrays"] == ["I_rank1.npy", "D_rank1.npy"]
    assert np.array_equal(np.load(tmp_path / "e" / "I_rank1.npy"), gI)


def test_verify_sample_poisons_before_its_step():
    """The sampled pairs are poisoned before the verifying step: a step that
    rewrites them passes, one that skips them (a replay that dropped a
    kernel family) fails."""
    cfg = dict(length=3000, p_max=0.01, cfg=2, k=21, protein=False)
    n = 6
    g = [bytes(r) for r in synth.genomes(n, cfg["length"], cfg["p_max"], cfg["cfg"])]
    off, codes = oracle.pack(g, 21, 0, 0)
    eI, eD = oracle.matrix(off, codes, 0, n, 0, n)
    ident = lambda v: v   # noqa: E731
    r0, r1 = 2, 5
    I = np.ascontiguousarray(eI[r0:r1].astype(np.int32)).ravel()
    D = np.ascontiguousarray(eD[r0:r1]).ravel()
    bI, bD = _FakeBuf(I.copy()), _FakeBuf(D.copy())

    def full_step():
        bI.arr[:] = I
        bD.arr[:] = D
    res = bench.verify_sample(cfg, "bitset", n, r0, r1, bI, bD, ident, step=full_step)
    assert res["ok"] and res["poisoned"]
    res = bench.verify_sample(cfg, "bitset", n, r0, r1, bI, bD, ident, step=lambda: None)
    assert not res["ok"]
