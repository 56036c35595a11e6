"""Host-side mirror of the reference's kmer-set API over libgdist.so.

Reference surface (org.theseed:sequence, un-vendored; call sites in-repo):
  KmerType.DNA / KmerType.PROT, getKmerSize(), createKmers(seq, K)
      FastaDistanceProcessor.java:81-96,153,184
  SequenceKmers.distance(other), size(), hashSet(width)
      FastaDistanceProcessor.java:186, SketchProcessor.java:88, WidthProcessor.java:178
  Sketch(int[] signature, name).distance(other), getSignature()
      WidthProcessor.java:178-185
The GPU-native form of these is a *collection*: `KmerSets` holds many kmer
sets packed on the device and answers whole matrices / row queries in one
call; `SequenceKmers` is a per-set view whose `distance()` is kept for API
parity (one pair per call is a correctness path, not a fast path).
"""
from __future__ import annotations

import contextlib
import ctypes as C
import enum
import math
import os
import weakref
from typing import Iterable, Mapping, Sequence

import numpy as np

from . import _lib as L


def option_names() -> list[str]:
    """Every tuning option of gdist_ctx_set_option (include/gdist.h)."""
    names, i = [], 0
    while True:
        p = C.c_char_p()
        if L.lib.gdist_ctx_option_name(i, C.byref(p)) != L.OK:
            return names
        names.append(p.value.decode())
        i += 1


def options_from_env(environ: Mapping[str, str] | None = None) -> dict[str, int]:
    """GDIST_<NAME>=<int> variables of a host program's environment as an
    options dict. The library itself never reads the environment; A/B
    launchers (bench.py, scripts/) map it explicitly with this."""
    env = os.environ if environ is None else environ
    out = {}
    for name in option_names():
        v = env.get("GDIST_" + name.upper())
        if v is not None and v != "":
            out[name] = int(v)
    return out


class Context:
    """One HIP device + stream (gdist_ctx) and its tuning options."""

    _defaults: dict[int, "Context"] = {}

    def __init__(self, device: int = 0, options: Mapping[str, int] | None = None):
        h = C.c_void_p()
        L.check(L.lib.gdist_ctx_create(device, C.byref(h)))
        self.h = h
        self.device = device
        self._handles = weakref.WeakSet()     # live collections: freed before the context
        for k, v in (options or {}).items():
            self.set_option(k, v)

    def set_option(self, name: str, value: int | None) -> None:
        """gdist_ctx_set_option; None restores the default."""
        L.check(L.lib.gdist_ctx_set_option(self.h, name.encode(), L.OPTION_DEFAULT if value is None else int(value)))

    def option(self, name: str) -> int | None:
        """The option's value, None when it is at its default."""
        v, is_set = C.c_int64(), C.c_int()
        L.check(L.lib.gdist_ctx_get_option(self.h, name.encode(), C.byref(v), C.byref(is_set)))
        return int(v.value) if is_set.value else None

    @contextlib.contextmanager
    def options(self, **opts: int | None):
        """Set options for the duration of a with-block, then restore them."""
        old = {k: self.option(k) for k in opts}
        try:
            for k, v in opts.items():
                self.set_option(k, v)
            yield self
        finally:
            for k, v in old.items():
                self.set_option(k, v)

    @classmethod
    def default(cls, device: int = 0) -> "Context":
        if device not in cls._defaults:
            cls._defaults[device] = cls(device)
        return cls._defaults[device]

    def close(self):
        """gdist_ctx_destroy, after freeing every collection still alive on it
        (a collection must not outlive its context)."""
        if self.h:
            for hd in list(self._handles):
                hd.free()
            L.lib.gdist_ctx_destroy(self.h)
            self.h = None

    def synchronize(self):
        L.check(L.lib.gdist_ctx_synchronize(self.h))

    def last_timing(self) -> tuple[float, float, int]:
        k, c, n = C.c_double(), C.c_double(), C.c_int64()
        L.check(L.lib.gdist_ctx_last_timing(self.h, C.byref(k), C.byref(c), C.byref(n)))
        return k.value, c.value, n.value

    KERNEL_FAMILIES = {"sparse": 0, "rare": 1, "dense": 2, "sorted": 3, "variant": 4}

    def kernel_ms(self, family: str) -> float:
        """HIP-event ms of one kernel family's launches (sparse / rare / dense /
        sorted) in the last call made with option time_kernels = 1 (-1: that
        family was not timed)."""
        v = C.c_double()
        L.check(L.lib.gdist_ctx_kernel_ms(self.h, self.KERNEL_FAMILIES[family], C.byref(v)))
        return v.value

    def closest_timing(self) -> tuple[float, float]:
        """(matrix kernels ms, select kernel ms) of the last closest() call made
        with option time_kernels = 1, summed over its steps (-1: not timed)."""
        m, s = C.c_double(), C.c_double()
        L.check(L.lib.gdist_ctx_closest_timing(self.h, C.byref(m), C.byref(s)))
        return m.value, s.value

    def group_stats_timing(self) -> tuple[float, float]:
        """(matrix kernels ms, reduce kernel ms) of the last group_stats() call
        made with option time_kernels = 1, summed over its steps (-1: not timed)."""
        m, s = C.c_double(), C.c_double()
        L.check(L.lib.gdist_ctx_group_stats_timing(self.h, C.byref(m), C.byref(s)))
        return m.value, s.value

    def within_timing(self) -> tuple[float, float]:
        """(matrix kernels ms, count + scan + write kernels ms) of the last
        within() call made with option time_kernels = 1, summed over its steps
        (-1: not timed)."""
        m, s = C.c_double(), C.c_double()
        L.check(L.lib.gdist_ctx_within_timing(self.h, C.byref(m), C.byref(s)))
        return m.value, s.value

    def histogram_timing(self) -> tuple[float, float]:
        """(matrix kernels ms, histogram kernel ms) of the last histogram() call
        made with option time_kernels = 1, summed over its steps (-1: not timed)."""
        m, s = C.c_double(), C.c_double()
        L.check(L.lib.gdist_ctx_histogram_timing(self.h, C.byref(m), C.byref(s)))
        return m.value, s.value

    def cross_info(self) -> tuple[float, float, int]:
        """(join kernel ms, select kernel ms, units) of the context's last
        cross_*() call (gdist_ctx_cross_info): the times are summed over the
        steps and -1 unless option time_kernels = 1. The second one is the
        kernels that consume the counts: the select (cross_closest), the
        distance epilogue (cross_matrix), count + scan + write (cross_within),
        the reduce (cross_group_stats), the histogram kernel (cross_histogram).
        units are the (query row, column block, segment range) work units launched."""
        j, s, u = C.c_double(), C.c_double(), C.c_int64()
        L.check(L.lib.gdist_ctx_cross_info(self.h, C.byref(j), C.byref(s), C.byref(u)))
        return j.value, s.value, u.value

    def reps_info(self) -> tuple[int, int, int, int]:
        """The context's last SketchSets.greedy_reps() call (gdist_ctx_reps_info):
        (row blocks of pass 1, (row, representative) cells the column-list
        launches covered in pass 1, the same for pass 2 (0 without assign),
        column-list launches). Zeros before any such call."""
        out = (C.c_int64 * 4)()
        L.check(L.lib.gdist_ctx_reps_info(self.h, out))
        return tuple(int(v) for v in out)

    def step_info(self) -> tuple[int, int, int, int]:
        """How the context's repeated matrix_device() calls went out so far
        (gdist_ctx_step_info): (fused sparse steps issued pipelined over the
        three streams, those of them fully ordered behind the context's stream
        first, steps replayed as one graph, bytes of second buffer copies held)."""
        out = (C.c_int64 * 4)()
        L.check(L.lib.gdist_ctx_step_info(self.h, out))
        return tuple(int(x) for x in out)

    def recent_timings(self, n: int) -> list[float]:
        """Kernel ms of the last n matrix calls, oldest first (waits for them)."""
        out = np.zeros(max(n, 1), dtype=np.float64)
        cnt = C.c_int()
        L.check(L.lib.gdist_ctx_recent_timings(self.h, int(n), L.ptr(out, C.c_double), C.byref(cnt)))
        return [float(x) for x in out[:cnt.value]]

    def alloc(self, nbytes: int) -> "DeviceBuffer":
        return DeviceBuffer(self, nbytes)

    # ---- RCCL communicator (row-sharded multi-GPU)
    @staticmethod
    def unique_id() -> bytes:
        buf = C.create_string_buffer(L.UNIQUE_ID_BYTES)
        L.check(L.lib.gdist_comm_unique_id(buf))
        return buf.raw

    def comm_init(self, uid: bytes, nranks: int, rank: int) -> None:
        L.check(L.lib.gdist_comm_init(self.h, uid, nranks, rank))

    def comm_init_host(self, nranks: int, rank: int, allgather) -> None:
        """Host-staged transport (gdist_comm_init_host): `allgather(np.uint8
        array of n bytes) -> np.uint8 array of nranks * n bytes in rank order`,
        e.g. torch.distributed.all_gather over gloo. For ranks sharing one GPU
        (RCCL refuses that) and tests; RCCL is the multi-GPU transport."""
        def cb(send, recv, nbytes, _user):
            try:
                src = np.ctypeslib.as_array((C.c_uint8 * max(int(nbytes), 1)).from_address(send))[:nbytes]
                out = np.ascontiguousarray(allgather(src.copy()), dtype=np.uint8)
                if out.nbytes != nbytes * nranks:
                    return 1
                if out.nbytes:
                    C.memmove(recv, out.ctypes.data, out.nbytes)
                return 0
            except Exception:
                return 1
        self._host_ag = L.ALLGATHER_FN(cb)          # keep the thunk alive
        L.check(L.lib.gdist_comm_init_host(self.h, nranks, rank, C.cast(self._host_ag, C.c_void_p), None))

    def comm_destroy(self) -> None:
        L.check(L.lib.gdist_comm_destroy(self.h))
        self._host_ag = None

    def allreduce_max(self, v: float) -> float:
        x = C.c_double(v)
        L.check(L.lib.gdist_comm_allreduce_max(self.h, C.byref(x)))
        return x.value


def release_device_cache(device: int = 0) -> None:
    """gdist_release_cache: hand the library's cached device blocks back to
    the driver (before another process takes the GPU)."""
    L.check(L.lib.gdist_release_cache(int(device)))


class HostBuffer:
    """Page-locked host memory (gdist_host_alloc) for sequence bytes: fill
    `array` (uint8) in place, e.g. with a FASTA reader, and pass it to
    KmerSets.from_blob: the pack uploads it with one DMA per chunk instead of
    the runtime's staged pageable copies. `array` must not be used after
    free() / the with-block."""

    def __init__(self, nbytes: int):
        p = C.c_void_p()
        L.check(L.lib.gdist_host_alloc(int(nbytes), C.byref(p)))
        self.ptr, self.nbytes = p.value or 0, int(nbytes)
        self.array = np.ctypeslib.as_array((C.c_uint8 * max(1, self.nbytes)).from_address(self.ptr))[:self.nbytes]

    def free(self):
        if self.ptr:
            self.array = None
            L.check(L.lib.gdist_host_free(self.ptr))
            self.ptr = 0

    def __enter__(self):
        return self

    def __exit__(self, *exc):
        self.free()

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class DeviceBuffer:
    def __init__(self, ctx: Context, nbytes: int):
        p = C.c_void_p()
        L.check(L.lib.gdist_dev_alloc(ctx.h, int(nbytes), C.byref(p)))
        self.ctx, self.ptr, self.nbytes = ctx, p.value or 0, int(nbytes)
        ctx._handles.add(self)

    def to_host(self, dtype, count: int | None = None, offset: int = 0) -> np.ndarray:
        """`count` elements of `dtype` starting at element `offset`."""
        dt = np.dtype(dtype)
        n = (self.nbytes // dt.itemsize - offset) if count is None else count
        if offset < 0 or n < 0 or (offset + n) * dt.itemsize > self.nbytes:
            raise ValueError("read outside the device buffer")
        out = np.empty(n, dtype=dt)
        L.check(L.lib.gdist_memcpy_d2h(self.ctx.h, out.ctypes.data, self.ptr + offset * dt.itemsize,
                                       n * dt.itemsize))
        return out

    def from_host(self, a: np.ndarray, offset: int = 0):
        """Copy `a` into the buffer from element `offset` (in a's dtype) on."""
        a = np.ascontiguousarray(a)
        at = int(offset) * a.itemsize
        if offset < 0 or at + a.nbytes > self.nbytes:
            raise ValueError("write outside the device buffer")
        L.check(L.lib.gdist_memcpy_h2d(self.ctx.h, self.ptr + at, a.ctypes.data, a.nbytes))

    def free(self):
        if self.ptr:
            L.check(L.lib.gdist_dev_free(self.ctx.h, self.ptr))
            self.ptr = 0

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass


class KmerType(enum.Enum):
    """KmerType.DNA / KmerType.PROT (FastaDistanceProcessor.java:81-96)."""
    DNA = (L.DNA, 21)
    PROT = (L.PROT, 8)

    @property
    def kind(self) -> int:
        return self.value[0]

    def getKmerSize(self) -> int:
        return self.value[1]

    def createKmers(self, seq: str | bytes, k: int, flags: int = 0, ctx: Context | None = None) -> "SequenceKmers":
        return KmerSets.from_sequences([seq], k, self, flags, ctx)[0]

    @classmethod
    def parse(cls, name: str) -> "KmerType":
        return cls[name.upper()]


def _as_bytes(s) -> bytes:
    return s if isinstance(s, (bytes, bytearray)) else str(s).encode("latin-1")


class GroupStats:
    """Result of group_stats (gdist_group_stats): for each of T groupings the
    in-group (column 0) and out-group (column 1) summary of the distances.

    n, ones, nans: int64 [T, 2] (values below 1.0 summarised, distances equal
    to 1.0, NaNs); min, max, mean, sdev: float64 [T, 2] (1.0 / 1.0 / 1.0 / 0.0
    for a side with n == 0); bad: int64 [T] pairs with an unlabelled set;
    sum, sumsq: [T][2] Python ints, the exact sums of m = d * 2^53 and m * m.
    `sides` / `bad_raw` are the C arrays (gdist_group_side [2 T], int64 [T])."""

    def __init__(self, sides, bad):
        self.sides, self.bad_raw = sides, bad
        T = len(bad)
        self.ntypes = T

        def arr(name, dtype):
            return np.array([[getattr(sides[2 * t + k], name) for k in range(2)] for t in range(T)], dtype=dtype)
        self.n, self.ones, self.nans = arr("n", np.int64), arr("ones", np.int64), arr("nans", np.int64)
        self.min, self.max = arr("min", np.float64), arr("max", np.float64)
        self.mean, self.sdev = arr("mean", np.float64), arr("sdev", np.float64)
        self.bad = np.array(list(bad), dtype=np.int64)

        def limbs(v):
            return sum(int(x) << (64 * i) for i, x in enumerate(v))
        self.sum = [[limbs(sides[2 * t + k].sum) for k in range(2)] for t in range(T)]
        self.sumsq = [[limbs(sides[2 * t + k].sumsq) for k in range(2)] for t in range(T)]

    @classmethod
    def empty(cls, ntypes: int) -> "GroupStats":
        """No pair yet: every side in its n == 0 form (the identity of merge)."""
        sides = (L.GroupSide * (2 * ntypes))()
        for s in sides:
            s.min = s.max = s.mean = 1.0
        return cls(sides, (C.c_int64 * ntypes)())

    def tobytes(self) -> bytes:
        """The struct array and the bad counts as the library wrote them."""
        return bytes(self.sides) + bytes(self.bad_raw)

    @classmethod
    def frombytes(cls, data: bytes) -> "GroupStats":
        """The summary tobytes() wrote (another rank's, received as bytes)."""
        per = 2 * C.sizeof(L.GroupSide) + 8
        T = len(data) // per
        if T < 1 or T * per != len(data):
            raise ValueError(f"{len(data)} bytes are not a whole number of groupings ({per} bytes each)")
        sides = (L.GroupSide * (2 * T)).from_buffer_copy(data[:T * (per - 8)])
        return cls(sides, (C.c_int64 * T).from_buffer_copy(data[T * (per - 8):]))

    def merge(self, other: "GroupStats") -> "GroupStats":
        """This summary and `other`'s (disjoint pairs, the same groupings) as
        one, exactly (gdist_group_stats_merge): the ranks of a row-sharded run
        merge to the bytes of a single call."""
        if other.ntypes != self.ntypes:
            raise ValueError("summaries of different groupings")
        T = self.ntypes
        sides, bad = (L.GroupSide * (2 * T))(), (C.c_int64 * T)()
        C.memmove(sides, self.sides, C.sizeof(sides))
        C.memmove(bad, self.bad_raw, C.sizeof(bad))
        L.check(L.lib.gdist_group_stats_merge(C.addressof(sides), bad, C.addressof(other.sides), other.bad_raw, T))
        return GroupStats(sides, bad)

    @property
    def low(self) -> np.ndarray:
        """mean - sdev, fp64 (DistanceCheckProcessor.java:216-217)."""
        return self.mean - self.sdev

    @property
    def high(self) -> np.ndarray:
        """mean + sdev, fp64 (DistanceCheckProcessor.java:216,218)."""
        return self.mean + self.sdev


class WidthSweep:
    """Result of width_sweep (gdist_width_sweep): the error of the sketch
    distance against the exact one at each of S sketch sizes.

    pairs: the pairs i < j with exact distance < 1.0. Per size k: size int32
    [S]; dwarves int64 [S] (signatures shorter than the size); differing int64
    [S] (pairs whose two distances differ); max_err, total, mean float64 [S]
    (the largest relative error, their sum, total / pairs; 0.0 without
    pairs); sum: [S] Python ints, the exact sum of rint(e * 2^62). `rows` is
    the C array (gdist_width_row [S])."""

    def __init__(self, rows, pairs: int):
        self.rows, self.pairs = rows, int(pairs)

        def arr(name, dtype):
            return np.array([getattr(r, name) for r in rows], dtype=dtype)
        self.size = arr("size", np.int32)
        self.dwarves, self.differing = arr("dwarves", np.int64), arr("differing", np.int64)
        self.max_err, self.total, self.mean = (arr("max_err", np.float64), arr("total", np.float64),
                                               arr("mean", np.float64))
        self.sum = [int(r.sum[0]) | (int(r.sum[1]) << 64) for r in rows]

    def __len__(self) -> int:
        return len(self.rows)

    def tobytes(self) -> bytes:
        """The struct array and the pair count as the library wrote them."""
        return bytes(self.rows) + self.pairs.to_bytes(8, "little", signed=True)


class Histogram:
    """Result of histogram (gdist_histogram): how the distances of a region are
    distributed over E ascending bucket edges.

    edges: float64 [E]; counts: int64 [S, E + 1], counts[s, b] the pairs of
    series s with edges[b - 1] <= d < edges[b] (bucket 0: d < edges[0], bucket
    E: d >= edges[E - 1]); nans: int64 [S], the NaN pairs, in no bucket; bad:
    int64 [T], pairs with an unlabelled set. Without labels S = 1 and T = 0;
    with T groupings S = 2 T, series 2 t in-group and 2 t + 1 out-group.
    Every field is an exact integer count: histograms of disjoint regions with
    the same edges and labels add (`a + b`)."""

    def __init__(self, edges, counts, nans, bad):
        self.edges = np.ascontiguousarray(edges, dtype=np.float64)
        self.counts = np.ascontiguousarray(counts, dtype=np.int64)
        self.nans = np.ascontiguousarray(nans, dtype=np.int64)
        self.bad = np.ascontiguousarray(bad, dtype=np.int64)

    @property
    def total(self) -> np.ndarray:
        """int64 [S]: the pairs of every series (all buckets and the NaNs)."""
        return self.counts.sum(axis=1) + self.nans

    def tobytes(self) -> bytes:
        """counts, nans and bad as the library wrote them."""
        return self.counts.tobytes() + self.nans.tobytes() + self.bad.tobytes()

    def __add__(self, other: "Histogram") -> "Histogram":
        if not isinstance(other, Histogram):
            return NotImplemented
        if self.edges.tobytes() != other.edges.tobytes():
            raise ValueError("histograms over different edges")
        if self.counts.shape != other.counts.shape or self.bad.shape != other.bad.shape:
            raise ValueError("histograms of different shapes")
        return Histogram(self.edges, self.counts + other.counts, self.nans + other.nans, self.bad + other.bad)


_BITS_ONE = 0x3FF0000000000000      # the pattern of 1.0: d >= 0 is ordered by its unsigned pattern


class _Handle:
    def __init__(self, ctx: Context, h: C.c_void_p):
        self.ctx, self.h = ctx, h
        ctx._handles.add(self)

    def free(self):
        if getattr(self, "h", None):
            L.lib.gdist_sets_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def info(self):
        kind, k, n, t = C.c_int(), C.c_int(), C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_sets_info(self.h, C.byref(kind), C.byref(k), C.byref(n), C.byref(t)))
        return kind.value, k.value, n.value, t.value

    def __len__(self) -> int:
        return self.info()[2]

    def _closest(self, n: int, max_dist: float, rows, cols, method: int, flags: int, keep_self: bool):
        """gdist_closest over rows x cols: (idx[nr, n] int64, d[nr, n] float64, count[nr] int32)."""
        ns = len(self)
        r0, r1 = rows or (0, ns)
        c0, c1 = cols or (0, ns)
        nr = max(r1 - r0, 0)
        idx = np.full((nr, max(n, 0)), -1, dtype=np.int64)
        d = np.ones((nr, max(n, 0)), dtype=np.float64)
        cnt = np.zeros(nr, dtype=np.int32)
        # non-empty buffers behind empty results: the library is never handed a null output
        bi = idx if idx.size else np.zeros(1, dtype=np.int64)
        bd = d if d.size else np.zeros(1, dtype=np.float64)
        bc = cnt if cnt.size else np.zeros(1, dtype=np.int32)
        fl = flags | (L.CLOSEST_KEEP_SELF if keep_self else 0)
        L.check(L.lib.gdist_closest(self.ctx.h, self.h, r0, r1, c0, c1, method, fl, int(n), float(max_dist),
                                    L.ptr(bi, C.c_int64), L.ptr(bd, C.c_double), L.ptr(bc, C.c_int32)))
        return idx, d, cnt

    def _group_stats(self, labels, rows, cols, upper: bool, method: int, flags: int) -> GroupStats:
        ns = len(self)
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim == 1:
            lab = lab[None, :]
        if lab.ndim != 2 or lab.shape[1] != ns:
            raise ValueError(f"labels must be [T, {ns}] or [{ns}], not {list(lab.shape)}")
        T = lab.shape[0]
        if not 1 <= T <= L.GROUP_MAX_TYPES:
            raise ValueError(f"{T} groupings: 1 .. {L.GROUP_MAX_TYPES} a call")
        r0, r1 = rows or (0, ns)
        c0, c1 = cols or (0, ns)
        sides, bad = (L.GroupSide * (2 * T))(), (C.c_int64 * T)()
        buf = lab if lab.size else np.zeros(1, dtype=np.int32)
        fl = flags | (L.UPPER_TRIANGLE if upper else 0)
        L.check(L.lib.gdist_group_stats(self.ctx.h, self.h, r0, r1, c0, c1, method, fl, T, L.ptr(buf, C.c_int32),
                                        C.addressof(sides), bad))
        return GroupStats(sides, bad)

    def _histogram(self, edges, labels, rows, cols, upper: bool, method: int, flags: int) -> Histogram:
        ns = len(self)
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if not 1 <= len(e) <= L.HIST_MAX_EDGES:
            raise ValueError(f"{len(e)} edges: 1 .. {L.HIST_MAX_EDGES} a call")
        if labels is None:
            lab, T = None, 0
        else:
            lab = np.ascontiguousarray(labels, dtype=np.int32)
            if lab.ndim == 1:
                lab = lab[None, :]
            if lab.ndim != 2 or lab.shape[1] != ns:
                raise ValueError(f"labels must be [T, {ns}] or [{ns}], not {list(lab.shape)}")
            T = lab.shape[0]
            if not 1 <= T <= L.GROUP_MAX_TYPES:
                raise ValueError(f"{T} groupings: 1 .. {L.GROUP_MAX_TYPES} a call")
            if not lab.size:
                lab = np.zeros((T, 1), dtype=np.int32)
        r0, r1 = rows or (0, ns)
        c0, c1 = cols or (0, ns)
        S = 2 * T if T else 1
        counts = np.zeros((S, len(e) + 1), dtype=np.int64)
        nans = np.zeros(S, dtype=np.int64)
        bad = np.zeros(max(T, 1), dtype=np.int64)
        fl = flags | (L.UPPER_TRIANGLE if upper else 0)
        L.check(L.lib.gdist_histogram(self.ctx.h, self.h, r0, r1, c0, c1, method, fl, len(e), L.ptr(e, C.c_double),
                                      T, L.ptr(lab, C.c_int32) if T else None, L.ptr(counts, C.c_int64),
                                      L.ptr(nans, C.c_int64), L.ptr(bad, C.c_int64) if T else None))
        return Histogram(e, counts, nans, bad[:T])

    def _quantiles(self, q, rows, cols, upper: bool, method: int, flags: int):
        """Exact order statistics from histogram calls alone. d >= 0 and never
        -0.0, so its unsigned bit pattern orders it: per quantile an inclusive
        pattern interval [lo, hi] that holds the value of rank k. Every call
        cuts each unfinished interval into equal pattern ranges with its share
        of the 1023 edges and keeps the range that holds rank k (the counts
        below every edge are the cumulative sums of the buckets)."""
        qs = np.atleast_1d(np.asarray(q, dtype=np.float64)).reshape(-1)
        if len(qs) > 8:
            raise ValueError(f"{len(qs)} quantiles: at most 8 a call")
        if len(qs) and not np.all((qs >= 0.0) & (qs <= 1.0)):     # NaN fails too
            raise ValueError("a quantile outside [0, 1]")
        out = np.full(len(qs), np.nan, dtype=np.float64)
        if not len(qs):
            return out, 0, 0
        # invariant per quantile: fewer than k values lie below lo, at least k at or below hi
        iv = [[0, _BITS_ONE] for _ in qs]
        rank, n, calls = None, 0, 0
        while any(lo < hi for lo, hi in iv):
            # distinct unfinished intervals (in the first call all are one: [0.0, 1.0])
            todo = sorted({(lo, hi) for lo, hi in iv if lo < hi})
            share = L.HIST_MAX_EDGES // len(todo)
            pats = set()
            for lo, hi in todo:
                m = hi - lo + 1                       # patterns; pieces of at most ceil(m / (share + 1))
                pieces = min(m, share + 1)
                pats.update(lo + (i * m + pieces - 1) // pieces for i in range(1, pieces))
            pats = np.array(sorted(pats), dtype=np.uint64)
            h = self._histogram(pats.view(np.float64), None, rows, cols, upper, method, flags)
            calls += 1
            below = np.cumsum(h.counts[0])            # below[i]: values < edge i (NaN is in no bucket)
            if rank is None:
                n = int(below[-1])
                if n == 0:
                    return out, 0, calls
                rank = [max(1, min(n, int(math.ceil(float(x) * n)))) for x in qs]
            for v, k in zip(iv, rank):
                lo, hi = v
                if lo == hi:
                    continue
                # edges a .. b - 1 lie in (lo, hi]; i: the first of them with at least k values below it
                a = int(np.searchsorted(pats, np.uint64(lo), side="right"))
                b = int(np.searchsorted(pats, np.uint64(hi), side="right"))
                i = a + int(np.searchsorted(below[a:b], k, side="left"))
                if i > a:
                    v[0] = int(pats[i - 1])
                if i < b:
                    v[1] = int(pats[i]) - 1
        return np.array([lo for lo, _ in iv], dtype=np.uint64).view(np.float64), n, calls

    # first capacity guess of within(capacity=None): entries a row of the call
    WITHIN_GUESS_PER_ROW = 64

    def _within(self, max_dist: float, rows, cols, upper: bool, method: int, flags: int, keep_self: bool,
                capacity: int | None):
        """gdist_within over rows x cols: (rowptr int64[nr + 1], cols int64[m], d float64[m]),
        m = min(total, capacity); capacity None: the complete list (a guess,
        then a second call when the total exceeds it)."""
        ns = len(self)
        r0, r1 = rows or (0, ns)
        c0, c1 = cols or (0, ns)
        nr = max(r1 - r0, 0)
        fl = flags | (L.UPPER_TRIANGLE if upper else 0) | (L.CLOSEST_KEEP_SELF if keep_self else 0)
        rowptr = np.zeros(nr + 1, dtype=np.int64)
        total = C.c_int64(0)
        cap = int(capacity) if capacity is not None else max(nr, 1) * self.WITHIN_GUESS_PER_ROW
        while True:
            # non-empty buffers behind empty results: the library is never handed a null output
            col = np.zeros(max(cap, 1), dtype=np.int64)
            d = np.zeros(max(cap, 1), dtype=np.float64)
            L.check(L.lib.gdist_within(self.ctx.h, self.h, r0, r1, c0, c1, method, fl, float(max_dist), cap,
                                       L.ptr(rowptr, C.c_int64), L.ptr(col, C.c_int64), L.ptr(d, C.c_double),
                                       C.byref(total)))
            if capacity is not None or total.value <= cap:
                m = min(total.value, cap)
                return rowptr, col[:m], d[:m]
            cap = total.value

    # the gdist_cross_* calls behind KmerSets.cross_* and SketchSets.cross_*: `queries` (rows) against this
    # resident collection (cols)
    def _pairs(self, call, sets, rows, cols, args, want_I: bool, want_D: bool):
        """A pair-list call (gdist_pairs, gdist_cross_pairs, gdist_sketch_pairs): call(ctx, self,
        *sets, n, rows, cols, *args, I, D) -> (I int32[P] | None, D float64[P] | None)."""
        r = np.ascontiguousarray(rows, dtype=np.int64).reshape(-1)
        c = np.ascontiguousarray(cols, dtype=np.int64).reshape(-1)
        if len(r) != len(c):
            raise ValueError(f"{len(r)} rows but {len(c)} cols")
        n = len(r)
        I = np.full(n, -1, dtype=np.int32) if want_I else None
        D = np.full(n, np.nan, dtype=np.float64) if want_D else None
        L.check(call(self.ctx.h, self.h, *sets, n, L.ptr(r, C.c_int64) if n else None,
                     L.ptr(c, C.c_int64) if n else None, *args, L.ptr(I, C.c_int32) if want_I and n else None,
                     L.ptr(D, C.c_double) if want_D and n else None))
        return I, D

    def pairs_info(self) -> tuple[float, int, int]:
        """(kernel ms, groups, units) of the context's last pair-list call
        (gdist_ctx_pairs_info): the kernel time is -1 unless option
        time_kernels = 1; groups are the distinct rows of the list, units the
        work units launched for them (sketches: the sum over the rows of
        ceil(pairs of the row / 64))."""
        ms, g, u = C.c_double(), C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_ctx_pairs_info(self.ctx.h, C.byref(ms), C.byref(g), C.byref(u)))
        return ms.value, g.value, u.value

    def _cross_matrix(self, queries, rows, cols, flags: int, want_I: bool, want_D: bool):
        r0, r1 = rows or (0, len(queries))
        c0, c1 = cols or (0, len(self))
        nr, nc = max(r1 - r0, 0), max(c1 - c0, 0)
        I = np.full((nr, nc), -1, dtype=np.int32) if want_I else None
        D = np.full((nr, nc), np.nan, dtype=np.float64) if want_D else None
        L.check(L.lib.gdist_cross_matrix(self.ctx.h, queries.h, self.h, r0, r1, c0, c1, flags,
                                         L.ptr(I, C.c_int32) if want_I else None,
                                         L.ptr(D, C.c_double) if want_D else None, max(nc, 1)))
        return I, D

    def _cross_closest(self, queries, n: int, max_dist: float, rows, cols, flags: int):
        r0, r1 = rows or (0, len(queries))
        c0, c1 = cols or (0, len(self))
        nr = max(r1 - r0, 0)
        idx = np.full((nr, max(n, 0)), -1, dtype=np.int64)
        d = np.ones((nr, max(n, 0)), dtype=np.float64)
        cnt = np.zeros(nr, dtype=np.int32)
        # non-empty buffers behind empty results: the library is never handed a null output
        bi = idx if idx.size else np.zeros(1, dtype=np.int64)
        bd = d if d.size else np.zeros(1, dtype=np.float64)
        bc = cnt if cnt.size else np.zeros(1, dtype=np.int32)
        L.check(L.lib.gdist_cross_closest(self.ctx.h, queries.h, self.h, r0, r1, c0, c1, flags, int(n),
                                          float(max_dist), L.ptr(bi, C.c_int64), L.ptr(bd, C.c_double),
                                          L.ptr(bc, C.c_int32)))
        return idx, d, cnt

    @staticmethod
    def _cross_labels(labels, n: int, what: str) -> np.ndarray:
        lab = np.ascontiguousarray(labels, dtype=np.int32)
        if lab.ndim == 1:
            lab = lab[None, :]
        if lab.ndim != 2 or lab.shape[1] != n:
            raise ValueError(f"{what} must be [T, {n}] or [{n}], not {list(lab.shape)}")
        if not 1 <= lab.shape[0] <= L.GROUP_MAX_TYPES:
            raise ValueError(f"{lab.shape[0]} groupings: 1 .. {L.GROUP_MAX_TYPES} a call")
        return lab

    def _cross_within(self, queries, max_dist: float, rows, cols, flags: int, capacity):
        r0, r1 = rows or (0, len(queries))
        c0, c1 = cols or (0, len(self))
        nr = max(r1 - r0, 0)
        rowptr = np.zeros(nr + 1, dtype=np.int64)
        total = C.c_int64(0)
        cap = int(capacity) if capacity is not None else max(nr, 1) * self.WITHIN_GUESS_PER_ROW
        while True:
            # non-empty buffers behind empty results: the library is never handed a null output
            col = np.zeros(max(cap, 1), dtype=np.int64)
            d = np.zeros(max(cap, 1), dtype=np.float64)
            L.check(L.lib.gdist_cross_within(self.ctx.h, queries.h, self.h, r0, r1, c0, c1, flags, float(max_dist), cap,
                                             L.ptr(rowptr, C.c_int64), L.ptr(col, C.c_int64), L.ptr(d, C.c_double),
                                             C.byref(total)))
            if capacity is not None or total.value <= cap:
                m = min(total.value, cap)
                return rowptr, col[:m], d[:m]
            cap = total.value

    def _cross_group_stats(self, queries, qlabels, slabels, rows, cols, flags: int) -> GroupStats:
        ql = self._cross_labels(qlabels, len(queries), "qlabels")
        sl = self._cross_labels(slabels, len(self), "slabels")
        if ql.shape[0] != sl.shape[0]:
            raise ValueError(f"{ql.shape[0]} query groupings but {sl.shape[0]} subject groupings")
        T = ql.shape[0]
        r0, r1 = rows or (0, len(queries))
        c0, c1 = cols or (0, len(self))
        sides, bad = (L.GroupSide * (2 * T))(), (C.c_int64 * T)()
        qb = ql if ql.size else np.zeros(1, dtype=np.int32)
        sb = sl if sl.size else np.zeros(1, dtype=np.int32)
        L.check(L.lib.gdist_cross_group_stats(self.ctx.h, queries.h, self.h, r0, r1, c0, c1,
                                              flags, T, L.ptr(qb, C.c_int32),
                                              L.ptr(sb, C.c_int32), C.addressof(sides), bad))
        return GroupStats(sides, bad)

    def _cross_histogram(self, queries, edges, qlabels, slabels, rows, cols, flags: int) -> Histogram:
        e = np.ascontiguousarray(edges, dtype=np.float64).reshape(-1)
        if not 1 <= len(e) <= L.HIST_MAX_EDGES:
            raise ValueError(f"{len(e)} edges: 1 .. {L.HIST_MAX_EDGES} a call")
        if (qlabels is None) != (slabels is None):
            raise ValueError("qlabels and slabels come together")
        T, qb, sb = 0, None, None
        if qlabels is not None:
            ql = self._cross_labels(qlabels, len(queries), "qlabels")
            sl = self._cross_labels(slabels, len(self), "slabels")
            if ql.shape[0] != sl.shape[0]:
                raise ValueError(f"{ql.shape[0]} query groupings but {sl.shape[0]} subject groupings")
            T = ql.shape[0]
            qb = ql if ql.size else np.zeros(1, dtype=np.int32)
            sb = sl if sl.size else np.zeros(1, dtype=np.int32)
        r0, r1 = rows or (0, len(queries))
        c0, c1 = cols or (0, len(self))
        S = 2 * T if T else 1
        counts = np.zeros((S, len(e) + 1), dtype=np.int64)
        nans = np.zeros(S, dtype=np.int64)
        bad = np.zeros(max(T, 1), dtype=np.int64)
        L.check(L.lib.gdist_cross_histogram(self.ctx.h, queries.h, self.h, r0, r1, c0, c1,
                                            flags, len(e), L.ptr(e, C.c_double), T,
                                            L.ptr(qb, C.c_int32) if T else None, L.ptr(sb, C.c_int32) if T else None,
                                            L.ptr(counts, C.c_int64), L.ptr(nans, C.c_int64),
                                            L.ptr(bad, C.c_int64) if T else None))
        return Histogram(e, counts, nans, bad[:T])

    def getClosest(self, n: int, max_dist: float, **kw) -> list[list[tuple[int, float]]]:
        """getClosest(kmers, n, maxDist) for every row of closest(n, max_dist, **kw)
        (MashProcessor.java:150, FindProcessor.java:110), exhaustively: per query
        [(set, distance)] nearest first (ties by index), at most n, distance <=
        max_dist — the shape of LSHIndex.getClosest."""
        idx, d, cnt = self.closest(n, max_dist, **kw)
        return [[(int(idx[q, r]), float(d[q, r])) for r in range(cnt[q])] for q in range(len(cnt))]

    def allgather(self, consume: bool = False):
        """Concatenation of every rank's local collection, in rank order
        (one RCCL all-gather of offsets, one in place of codes / signatures).
        consume=True releases this collection's device data once its codes
        are in the gather buffer (GDIST_ALLGATHER_CONSUME): peak memory is
        then (ranks + 1) x the largest shard instead of + 2 shards."""
        h = C.c_void_p()
        L.check(L.lib.gdist_sets_allgather_ex(self.ctx.h, self.h, L.ALLGATHER_CONSUME if consume else 0,
                                              C.byref(h)))
        return type(self)(self.ctx, h)

    def concat(self, other):
        """gdist_sets_concat: a new collection of this one's sets, then
        `other`'s (kmer sets of one kmer spec, or sketches of one width): a
        deep copy on the device, independent of both inputs."""
        h = C.c_void_p()
        L.check(L.lib.gdist_sets_concat(self.h, other.h, C.byref(h)))
        return type(self)(self.ctx, h)

    def exchange_plan(self, method: int = L.METHOD_AUTO) -> tuple[int, float, float]:
        """(method, bytes_bitsets, bytes_codes): the exchange every rank of the
        communicator takes for a row-sharded N x N (collective call):
        METHOD_BITSET = the dictionary exchange (allgather_bitsets),
        METHOD_SORTED = the code all-gather (allgather) for the sorted join."""
        m = C.c_int()
        bb, bc = C.c_double(), C.c_double()
        L.check(L.lib.gdist_sets_exchange_plan(self.ctx.h, self.h, method, C.byref(m), C.byref(bb), C.byref(bc)))
        return m.value, bb.value, bc.value


class KmerSets(_Handle):
    """A collection of kmer sets (sorted unique uint64 codes) resident in HBM."""

    pack_flags = 0   # the pack flags of from_sequences / from_blob / from_device (pack_like)

    @classmethod
    def from_sequences(cls, seqs: Sequence, k: int, kmer_type: KmerType = KmerType.DNA, flags: int = 0,
                       ctx: Context | None = None) -> "KmerSets":
        ctx = ctx or Context.default()
        bs = [_as_bytes(s) for s in seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs])
        blob = b"".join(bs) or b"\0"
        h = C.c_void_p()
        L.check(L.lib.gdist_sets_pack(ctx.h, kmer_type.kind, int(k), flags, blob, L.ptr(off, C.c_int64),
                                      len(bs), C.byref(h)))
        sets = cls(ctx, h)
        sets.pack_flags = flags
        return sets

    def pack_like(self, seqs: Sequence) -> "KmerSets":
        """A new collection of `seqs` packed with this collection's kind, k and
        pack flags (the flags it was packed with through this binding; 0 for a
        collection of uploaded codes): queries for cross_matrix / cross_closest."""
        kind, k, _, _ = self.info()
        return KmerSets.from_sequences(seqs, k, KmerType.DNA if kind == L.DNA else KmerType.PROT, self.pack_flags,
                                       self.ctx)

    def append(self, seqs: Sequence) -> int:
        """gdist_sets_append: pack `seqs` with this collection's kmer spec and
        append them as new sets; returns the index of the first one. Every
        derived representation is rebuilt on the next distance call."""
        bs = [_as_bytes(s) for s in seqs]
        off = np.zeros(len(bs) + 1, dtype=np.int64)
        if bs:
            off[1:] = np.cumsum([len(b) for b in bs])
        blob = b"".join(bs) or b"\0"
        first = C.c_int64()
        L.check(L.lib.gdist_sets_append(self.ctx.h, self.h, blob, L.ptr(off, C.c_int64), len(bs), C.byref(first)))
        return first.value

    @classmethod
    def from_blob(cls, blob, offsets, k: int, kmer_type: KmerType = KmerType.DNA, flags: int = 0,
                  ctx: Context | None = None) -> "KmerSets":
        """Sequences already laid out as one byte buffer (bytes / bytearray /
        uint8 array) with int64 offsets (n + 1): passed to gdist_sets_pack as
        they are, no per-sequence copies (FASTA bytes read into memory)."""
        ctx = ctx or Context.default()
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        n = len(off) - 1
        if isinstance(blob, np.ndarray):
            buf = np.ascontiguousarray(blob, dtype=np.uint8)
            ptr = buf.ctypes.data_as(C.c_char_p) if buf.size else b"\0"
        else:
            buf = blob if len(blob) else b"\0"
            ptr = buf if isinstance(buf, bytes) else (C.c_char * len(buf)).from_buffer(buf)
        h = C.c_void_p()
        L.check(L.lib.gdist_sets_pack(ctx.h, kmer_type.kind, int(k), flags, ptr, L.ptr(off, C.c_int64), n,
                                      C.byref(h)))
        sets = cls(ctx, h)
        sets.pack_flags = flags
        return sets

    @classmethod
    def from_device(cls, ctx: Context, d_seqs: int, d_off: int, nseqs: int, total_bytes: int, k: int,
                    kmer_type: KmerType = KmerType.DNA, flags: int = 0) -> "KmerSets":
        h = C.c_void_p()
        L.check(L.lib.gdist_sets_pack_device(ctx.h, kmer_type.kind, int(k), flags, d_seqs, d_off, nseqs,
                                             total_bytes, C.byref(h)))
        sets = cls(ctx, h)
        sets.pack_flags = flags
        return sets

    @classmethod
    def from_codes(cls, offsets: np.ndarray, codes: np.ndarray, k: int, kmer_type: KmerType = KmerType.DNA,
                   ctx: Context | None = None) -> "KmerSets":
        ctx = ctx or Context.default()
        off = np.ascontiguousarray(offsets, dtype=np.int64)
        cd = np.ascontiguousarray(codes, dtype=np.uint64)
        if cd.size == 0:
            cd = np.zeros(1, dtype=np.uint64)
        h = C.c_void_p()
        L.check(L.lib.gdist_sets_upload(ctx.h, kmer_type.kind, int(k), len(off) - 1, L.ptr(off, C.c_int64),
                                        L.ptr(cd, C.c_uint64), C.byref(h)))
        return cls(ctx, h)

    def sizes(self) -> np.ndarray:
        n = len(self)
        out = np.zeros(n, dtype=np.int64)
        L.check(L.lib.gdist_sets_sizes(self.h, L.ptr(out, C.c_int64)))
        return out

    def download(self) -> tuple[np.ndarray, np.ndarray]:
        _, _, n, t = self.info()
        off = np.zeros(n + 1, dtype=np.int64)
        codes = np.zeros(max(t, 1), dtype=np.uint64)
        L.check(L.lib.gdist_sets_download(self.h, L.ptr(off, C.c_int64), L.ptr(codes, C.c_uint64)))
        return off, codes[:t]

    def build_bitsets(self, keep_singletons: bool = False, rare_threshold: int = -1) -> tuple[int, int]:
        """Dense bitsets (+ rare-kmer posting lists, see include/gdist.h); returns (dense dictionary, W)."""
        L.check(L.lib.gdist_sets_build_bitsets_ex(self.h, L.BITSET_KEEP_SINGLETONS if keep_singletons else 0,
                                                  rare_threshold))
        return self.bitset_info()

    def release_codes(self) -> None:
        """Drop the codes of a collection whose bitsets are built (gdist_sets_release_codes)."""
        L.check(L.lib.gdist_sets_release_codes(self.h))

    def build_timing(self) -> dict:
        """The last bitset build (gdist_sets_build_timing): wall ms, the split stages'
        ms over all shares and of the largest share, the shares, and one rank's
        projected build (wall - split + largest share)."""
        b, sp, mx, n = C.c_double(), C.c_double(), C.c_double(), C.c_int()
        L.check(L.lib.gdist_sets_build_timing(self.h, C.byref(b), C.byref(sp), C.byref(mx), C.byref(n)))
        return {"build_ms": b.value, "split_ms": sp.value, "share_max_ms": mx.value, "shares": n.value,
                "rank_ms": b.value - sp.value + mx.value}

    def prepare(self, method: int = L.METHOD_AUTO, pairs: float = -1.0) -> tuple[int, float, float]:
        """Build the representation `method` needs for `pairs` pairs (-1: the whole
        triangle); returns (method a matrix call will run, bitset cost estimate s
        (-1 without bitsets), sorted cost estimate s). See gdist_sets_prepare."""
        m, cb, cs = C.c_int(), C.c_double(), C.c_double()
        L.check(L.lib.gdist_sets_prepare(self.ctx.h, self.h, method, float(pairs), C.byref(m), C.byref(cb),
                                         C.byref(cs)))
        return m.value, cb.value, cs.value

    def greedy_reps(self, max_dist: float, assign: bool = False, tie_rank: np.ndarray | None = None,
                    method: int = L.METHOD_AUTO):
        """Greedy representatives on the device (gdist_greedy_reps). Returns
        is_rep (int32[N]); with assign=True also (rep_of int64[N], rep_dist
        float64[N]): each set's closest representative, ties to the lowest
        tie_rank (default: index)."""
        n = len(self)
        is_rep = np.zeros(max(n, 1), dtype=np.int32)
        nreps = C.c_int64()
        rep_of = np.zeros(max(n, 1), dtype=np.int64) if assign else None
        rep_d = np.zeros(max(n, 1), dtype=np.float64) if assign else None
        tr = None
        if tie_rank is not None:
            tr = np.ascontiguousarray(tie_rank, dtype=np.int64)
            assert tr.shape == (n,)
        L.check(L.lib.gdist_greedy_reps(self.ctx.h, self.h, method, float(max_dist),
                                        L.ptr(tr, C.c_int64) if tr is not None else None, L.ptr(is_rep, C.c_int32),
                                        L.ptr(rep_of, C.c_int64) if assign else None,
                                        L.ptr(rep_d, C.c_double) if assign else None, C.byref(nreps)))
        if assign:
            return is_rep[:n], rep_of[:n], rep_d[:n]
        return is_rep[:n]

    def block_cost(self, rows: tuple[int, int], cols: tuple[int, int] | None = None,
                   upper: bool = True) -> tuple[float, int]:
        """(modelled seconds, rare kernel: 0 list-major / 1 row-major / -1 none)
        of one matrix call on the block (gdist_sets_block_cost)."""
        c = cols if cols is not None else (0, len(self))
        t, rk = C.c_double(), C.c_int()
        L.check(L.lib.gdist_sets_block_cost(self.h, rows[0], rows[1], c[0], c[1], 1 if upper else 0, C.byref(t),
                                            C.byref(rk)))
        return t.value, rk.value

    def sparse_info(self) -> tuple[int, int, int]:
        """(complement-sparse words, dense words left to the tiles, complement entries)."""
        a, b, c = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_sets_sparse_info(self.h, C.byref(a), C.byref(b), C.byref(c)))
        return a.value, b.value, c.value

    def variant_info(self) -> tuple[int, int, int, float]:
        """(kmers, words, entries, products) of the variant tier (gdist_sets_variant_info)."""
        a, b, c, d = C.c_int64(), C.c_int64(), C.c_int64(), C.c_double()
        L.check(L.lib.gdist_sets_variant_info(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d)))
        return a.value, b.value, c.value, d.value

    def variant_layout(self) -> tuple[int, int, int]:
        """(kmers a word, bytes a list member, largest row weight) of the
        variant tier (gdist_sets_variant_layout): (16, 4, w) for the grouped
        rare tier of <= 65,536 sets (option rare_group), (47, 8, 0) for C4's
        packed members, (64, 12, 0) unpacked."""
        wk, mb, rw = C.c_int(), C.c_int(), C.c_int64()
        L.check(L.lib.gdist_sets_variant_layout(self.h, C.byref(wk), C.byref(mb), C.byref(rw)))
        return wk.value, mb.value, rw.value

    def group_info(self) -> tuple[int, int]:
        """(groups, grouped sparse words) of the group tier (gdist_sets_group_info)."""
        g, w = C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_sets_group_info(self.h, C.byref(g), C.byref(w)))
        return g.value, w.value

    def sparse_sides(self) -> tuple[int, int]:
        """(complement-sparse words, positive-sparse words)."""
        a, b = C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_sets_sparse_sides(self.h, C.byref(a), C.byref(b)))
        return a.value, b.value

    def sparse_triples(self) -> tuple[int, int, int, int, int]:
        """(triple records, empty lists, lists with n mod 3 = 1, 2, 0 and n > 0) of the
        sparse words' (set block, word) lists (gdist_sets_sparse_triples)."""
        out = (C.c_int64 * 5)()
        L.check(L.lib.gdist_sets_sparse_triples(self.h, out))
        return tuple(int(v) for v in out)

    def sparse_pairs(self) -> float:
        """The sparse tile kernel's products: sum over sparse words of z (z - 1) / 2."""
        p = C.c_double()
        L.check(L.lib.gdist_sets_sparse_pairs(self.h, C.byref(p)))
        return p.value

    def rare_kmers(self) -> int:
        """Rare-tier kmers before identical posting lists were merged."""
        n = C.c_int64()
        L.check(L.lib.gdist_sets_rare_kmers(self.h, C.byref(n)))
        return n.value

    def rare_info(self) -> tuple[int, int, int]:
        """(threshold T, distinct posting lists, their records) of the rare tier."""
        t, n, r = C.c_int64(), C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_sets_rare_info(self.h, C.byref(t), C.byref(n), C.byref(r)))
        return t.value, n.value, r.value

    def rare_stats(self) -> tuple[int, int]:
        """(pair increments, longest posting list) of the rare tier."""
        i, m = C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_sets_rare_stats(self.h, C.byref(i), C.byref(m)))
        return i.value, m.value

    def bitsets(self) -> np.ndarray:
        """The dictionary-rank bitsets, (nsets, W) uint64."""
        n = len(self)
        _, w = self.bitset_info()
        out = np.zeros((n, max(w, 1)), dtype=np.uint64)
        L.check(L.lib.gdist_sets_bitset_download(self.h, L.ptr(out, C.c_uint64)))
        return out[:, :w]

    def bitset_info(self) -> tuple[int, int]:
        d, w = C.c_int64(), C.c_int64()
        L.check(L.lib.gdist_sets_bitset_info(self.h, C.byref(d), C.byref(w)))
        return d.value, w.value

    def allgather_bitsets(self, keep_singletons: bool = False) -> "KmerSets":
        """Bitsets of every rank's sets over one global dictionary (bitset-only collection)."""
        h = C.c_void_p()
        L.check(L.lib.gdist_sets_allgather_bitsets(self.ctx.h, self.h,
                                                   L.BITSET_KEEP_SINGLETONS if keep_singletons else 0,
                                                   C.byref(h)))
        return KmerSets(self.ctx, h)

    def matrix(self, rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
               upper: bool = False, method: int = L.METHOD_AUTO, flags: int = 0,
               want_I: bool = True, want_D: bool = True):
        """|A_i ∩ A_j| and distances for rows × cols (host numpy outputs)."""
        n = len(self)
        r0, r1 = rows or (0, n)
        c0, c1 = cols or (0, n)
        nr, nc = r1 - r0, c1 - c0
        I = np.full((nr, nc), -1, dtype=np.int32) if want_I else None
        D = np.full((nr, nc), np.nan, dtype=np.float64) if want_D else None
        fl = flags | (L.UPPER_TRIANGLE if upper else 0)
        L.check(L.lib.gdist_intersect_matrix(self.ctx.h, self.h, r0, r1, c0, c1, method, fl, L.vptr(I),
                                             L.vptr(D), max(nc, 1)))
        return I, D

    def matrix_device(self, d_I: int | None, d_D: int | None, ld: int, rows: tuple[int, int],
                      cols: tuple[int, int], upper: bool = False, method: int = L.METHOD_AUTO,
                      flags: int = 0) -> None:
        fl = flags | L.OUT_DEVICE | (L.UPPER_TRIANGLE if upper else 0)
        L.check(L.lib.gdist_intersect_matrix(self.ctx.h, self.h, rows[0], rows[1], cols[0], cols[1], method,
                                             fl, d_I, d_D, ld))

    def closest(self, n: int, max_dist: float, rows: tuple[int, int] | None = None,
                cols: tuple[int, int] | None = None, method: int = L.METHOD_AUTO, flags: int = 0,
                keep_self: bool = False):
        """Exact nearest neighbours (gdist_closest): for every set of `rows` the n
        sets of `cols` with the smallest Jaccard distance <= max_dist, ordered by
        (distance, index), the set itself left out unless keep_self. Returns
        (idx[nr, n] int64, d[nr, n] float64, count[nr] int32); unused slots are
        -1 / 1.0. d is bit-identical to matrix()'s D; the N x N stays on the device."""
        return self._closest(n, max_dist, rows, cols, method, flags, keep_self)

    def within(self, max_dist: float, rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
               upper: bool = False, method: int = L.METHOD_AUTO, flags: int = 0, keep_self: bool = False,
               capacity: int | None = None):
        """Every pair within a distance (gdist_within): the pairs (i, j) of rows x
        cols with Jaccard distance <= max_dist, row ascending then column
        ascending, as CSR: (rowptr int64[nr + 1], cols int64[m], d float64[m]).
        The set itself is left out unless keep_self; upper: only j > i.
        capacity None: the complete list; a number: at most that many entries
        (m = min(total, capacity)), rowptr still the full counts. d is
        bit-identical to matrix()'s D; the N x N stays on the device."""
        return self._within(max_dist, rows, cols, upper, method, flags, keep_self, capacity)

    def group_stats(self, labels, rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
                    upper: bool = True, method: int = L.METHOD_AUTO, flags: int = 0) -> GroupStats:
        """In-group / out-group summary of the distances of rows x cols
        (gdist_group_stats; GroupTypeSpec.java:77-95): labels int32 [T, N] or
        [N], the group of every set under each grouping (< 0: none, the pair
        is counted as bad). upper: only the pairs j > i. The distances are
        matrix()'s D bit for bit and never leave the device; the sums are
        exact, so the result does not depend on method or block sizes."""
        return self._group_stats(labels, rows, cols, upper, method, flags)

    def histogram(self, edges, labels=None, rows: tuple[int, int] | None = None,
                  cols: tuple[int, int] | None = None, upper: bool = True, method: int = L.METHOD_AUTO,
                  flags: int = 0) -> Histogram:
        """How the distances of rows x cols are distributed (gdist_histogram):
        edges float64 [E], strictly ascending, at most HIST_MAX_EDGES; a
        distance goes to bucket numpy.searchsorted(edges, d, "right"), NaN to
        `nans`. labels None: one series of every pair; int32 [T, N] or [N]:
        per grouping an in-group and an out-group series, split as group_stats
        splits them. upper: only the pairs j > i. The distances are matrix()'s
        D bit for bit and never leave the device; every count is exact."""
        return self._histogram(edges, labels, rows, cols, upper, method, flags)

    def quantiles(self, q, rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
                  upper: bool = True, method: int = L.METHOD_AUTO, flags: int = 0):
        """Exact order statistics of the non-NaN distances of rows x cols, from
        a few histogram() calls: (values float64 [len(q)], n, calls). With the
        n values sorted ascending as x_1..x_n the value for q in [0, 1] is x_k,
        k = max(1, min(n, ceil(q n))); n == 0 gives NaN. At most 8 quantiles a
        call: one finishes in at most 7 histogram calls, eight in at most 9."""
        return self._quantiles(q, rows, cols, upper, method, flags)

    def pairs(self, rows, cols, method: int = L.METHOD_AUTO, flags: int = 0, want_I: bool = True,
              want_D: bool = True, *, other: "KmerSets | None" = None):
        """Distances of a pair list (gdist_pairs): for every p the intersection
        count and distance of sets (rows[p], cols[p]), in one device call:
        (I int32[P] | None, D float64[P] | None). Any order, repeats and i == j
        allowed; both are matrix()'s I and D of that cell bit for bit.

        With `other` (gdist_cross_pairs) rows index this collection (the
        queries) and cols index `other` (the resident subjects, only read):
        other.cross_matrix(self)'s cell (rows[p], cols[p]) bit for bit. There
        is no bitset route across two collections: method must be AUTO or
        SORTED; flags: EMPTY_NAN or 0."""
        if other is None:
            return self._pairs(L.lib.gdist_pairs, (), rows, cols, (method, flags), want_I, want_D)
        if method not in (L.METHOD_AUTO, L.METHOD_SORTED):
            raise ValueError("a pair list across two collections runs the sorted join: method AUTO or SORTED")
        return self._pairs(L.lib.gdist_cross_pairs, (other.h,), rows, cols, (flags,), want_I, want_D)

    def cross_matrix(self, queries: "KmerSets", rows: tuple[int, int] | None = None,
                     cols: tuple[int, int] | None = None, flags: int = 0, want_I: bool = True,
                     want_D: bool = True):
        """|Q_i ∩ S_j| and distances of `queries` (rows) against this resident
        collection (cols), host numpy outputs (gdist_cross_matrix). This
        collection is only read (its segment index is built when absent) and
        nothing is packed again: bit for bit the rectangle matrix(method=
        METHOD_SORTED) gives for self.concat(queries). flags: EMPTY_NAN or 0."""
        return self._cross_matrix(queries, rows, cols, flags, want_I, want_D)

    def cross_closest(self, queries: "KmerSets", n: int, max_dist: float, rows: tuple[int, int] | None = None,
                      cols: tuple[int, int] | None = None, flags: int = 0):
        """Exact nearest neighbours of `queries` among this resident collection
        (gdist_cross_closest): for every query of `rows` the n sets of `cols`
        with the smallest Jaccard distance <= max_dist, ordered by (distance,
        index); no set is left out as the query itself. Returns (idx[nr, n]
        int64, d[nr, n] float64, count[nr] int32) laid out as closest() lays
        them out; d is cross_matrix()'s D bit for bit. This collection is only
        read and nothing is packed again."""
        return self._cross_closest(queries, n, max_dist, rows, cols, flags)

    def cross_within(self, queries: "KmerSets", max_dist: float, rows: tuple[int, int] | None = None,
                     cols: tuple[int, int] | None = None, empty_nan: bool = False, capacity: int | None = None):
        """Every (query, resident set) pair within a distance (gdist_cross_within):
        the pairs (i, j) of `rows` of `queries` x `cols` of this collection with
        Jaccard distance <= max_dist, row ascending then column ascending, as
        CSR: (rowptr int64[nr + 1], cols int64[m], d float64[m]); the columns
        are indices of this collection and none is left out as the query
        itself. capacity None: the complete list (a guess, then a second call
        when the total exceeds it, as within()); a number: at most that many
        entries, rowptr still the full counts. d is cross_matrix()'s D bit for
        bit. This collection is only read and nothing is packed again."""
        return self._cross_within(queries, max_dist, rows, cols, L.EMPTY_NAN if empty_nan else 0, capacity)

    def cross_group_stats(self, queries: "KmerSets", qlabels, slabels, rows: tuple[int, int] | None = None,
                          cols: tuple[int, int] | None = None, empty_nan: bool = False) -> GroupStats:
        """In-group / out-group summary of the distances of `queries` (rows)
        against this resident collection (cols) (gdist_cross_group_stats):
        qlabels int32 [T, len(queries)] and slabels int32 [T, len(self)] (or
        1-d for one grouping), the group of every set (< 0: none, the pair is
        counted as bad). Every cell of the rectangle counts. The result merges
        with any other GroupStats; this collection is only read."""
        return self._cross_group_stats(queries, qlabels, slabels, rows, cols, L.EMPTY_NAN if empty_nan else 0)

    def cross_histogram(self, queries: "KmerSets", edges, qlabels=None, slabels=None,
                        rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
                        empty_nan: bool = False) -> Histogram:
        """How the distances of `queries` (rows) against this resident
        collection (cols) are distributed (gdist_cross_histogram): edges and
        buckets as histogram(); without labels one series of every pair, with
        qlabels / slabels (as cross_group_stats) an in-group and an out-group
        series per grouping. Every cell of the rectangle counts; histograms of
        disjoint rectangles add. This collection is only read."""
        return self._cross_histogram(queries, edges, qlabels, slabels, rows, cols,
                                     L.EMPTY_NAN if empty_nan else 0)

    def row_query(self, q: int, cols: Iterable[int], mode: int = L.QUERY_ALL, t: float = 1.0):
        cl = np.ascontiguousarray(np.fromiter(cols, dtype=np.int64))
        D = np.zeros(max(len(cl), 1), dtype=np.float64)
        hit, bi, bd = C.c_int32(0), C.c_int64(-1), C.c_double(1.0)
        L.check(L.lib.gdist_row_query(self.ctx.h, self.h, q, L.ptr(cl, C.c_int64) if len(cl) else None,
                                      len(cl), mode, t, L.ptr(D, C.c_double), C.byref(hit), C.byref(bi),
                                      C.byref(bd)))
        if mode == L.QUERY_ANY_LE:
            return bool(hit.value)
        if mode == L.QUERY_ARGMIN:
            return int(bi.value), float(bd.value)
        return D[:len(cl)]

    def sketches(self, width: int) -> "SketchSets":
        h = C.c_void_p()
        L.check(L.lib.gdist_sketch_build(self.ctx.h, self.h, int(width), C.byref(h)))
        return SketchSets(self.ctx, h)

    def width_sweep(self, sk: "SketchSets", sizes, method: int = L.METHOD_AUTO, flags: int = 0) -> WidthSweep:
        """The error of the sketch distance at every sketch size of `sizes`
        (strictly increasing, at most WIDTH_MAX_SIZES) in one walk of the
        pairs (gdist_width_sweep; WidthProcessor.java:153-208). `sk` is
        self.sketches(W) for a W >= sizes[-1]: its signatures' prefixes are
        the sketches of every smaller size. flags: 0 or SKETCH_JACCARD. Every
        field is exact, so the result depends on neither method nor block
        sizes; neither distance table leaves the device."""
        sz = np.ascontiguousarray(np.asarray(sizes, dtype=np.int64).reshape(-1))
        if sz.size and (sz.min() < -2**31 or sz.max() >= 2**31):
            raise ValueError("a sketch size does not fit 32 bits")
        sz = sz.astype(np.int32)
        rows = (L.WidthRow * len(sz))()
        pairs = C.c_int64(0)
        L.check(L.lib.gdist_width_sweep(self.ctx.h, self.h, sk.h, len(sz), L.ptr(sz, C.c_int32) if len(sz) else None,
                                        int(method), int(flags), C.addressof(rows) if len(sz) else None,
                                        C.byref(pairs)))
        return WidthSweep(rows, pairs.value)

    def __getitem__(self, i: int) -> "SequenceKmers":
        n = len(self)
        if i < 0:
            i += n
        if not 0 <= i < n:
            raise IndexError(i)
        return SequenceKmers(self, i)


class SequenceKmers:
    """SequenceKmers view of one set of a KmerSets collection."""

    def __init__(self, sets: KmerSets, index: int):
        self.sets, self.index = sets, index

    def size(self) -> int:
        return int(self.sets.sizes()[self.index])

    def distance(self, other: "SequenceKmers") -> float:
        """SequenceKmers.distance(other) — FastaDistanceProcessor.java:186."""
        if other.sets is self.sets:
            return float(self.sets.row_query(self.index, [other.index])[0])
        # one cell against the other collection as it is: no copy of either (gdist_cross_pairs)
        _, D = self.sets.pairs([self.index], [other.index], want_I=False, other=other.sets)
        return float(D[0])

    def similarity(self, other: "SequenceKmers") -> int:
        if other.sets is self.sets:
            I, _ = self.sets.matrix((self.index, self.index + 1), (other.index, other.index + 1), want_D=False)
            return int(I[0, 0])
        I, _ = self.sets.pairs([self.index], [other.index], want_D=False, other=other.sets)
        return int(I[0])

    def hashSet(self, width: int) -> np.ndarray:
        """SequenceKmers.hashSet(width) — SketchProcessor.java:88."""
        return self.sets.sketches(width).signature(self.index)


def reduce_row_query(D, mode: int = L.QUERY_ALL, t: float = 1.0):
    """The reductions gdist_row_query documents, on a row of distances already
    on the host (SketchSets.row_query). ALL: the distances as they are. ANY_LE:
    True when any distance is <= t. ARGMIN: (position, distance) of the
    smallest distance, ties to the lowest position; (-1, 1.0) when no distance
    is below 1.0 (the reference's NULL_RESULT identity wins ties at 1.0).
    NaN never qualifies, in either mode."""
    D = np.asarray(D, dtype=np.float64).reshape(-1)
    if mode == L.QUERY_ALL:
        return D
    if mode == L.QUERY_ANY_LE:
        return bool(np.any(D <= t))            # a comparison with NaN is False
    if mode != L.QUERY_ARGMIN:
        raise ValueError(f"unknown row query mode {mode}")
    ok = D < 1.0
    if not ok.any():
        return -1, 1.0
    i = int(np.argmin(np.where(ok, D, np.inf)))   # the first of equal minima
    return i, float(D[i])


class SketchSets(_Handle):
    """Bottom-s MinHash signatures (int32) resident in HBM."""

    @classmethod
    def from_signatures(cls, sigs: Sequence[np.ndarray], width: int, ctx: Context | None = None) -> "SketchSets":
        ctx = ctx or Context.default()
        off = np.zeros(len(sigs) + 1, dtype=np.int64)
        if sigs:
            off[1:] = np.cumsum([len(s) for s in sigs])
        flat = np.concatenate([np.asarray(s, dtype=np.int32) for s in sigs]) if sigs else np.zeros(0, np.int32)
        if flat.size == 0:
            flat = np.zeros(1, dtype=np.int32)
        h = C.c_void_p()
        L.check(L.lib.gdist_sketch_upload(ctx.h, int(width), len(sigs), L.ptr(off, C.c_int64),
                                          L.ptr(np.ascontiguousarray(flat), C.c_int32), C.byref(h)))
        return cls(ctx, h)

    def download(self) -> tuple[np.ndarray, np.ndarray]:
        _, _, n, t = self.info()
        off = np.zeros(n + 1, dtype=np.int64)
        sig = np.zeros(max(t, 1), dtype=np.int32)
        L.check(L.lib.gdist_sketch_download(self.h, L.ptr(off, C.c_int64), L.ptr(sig, C.c_int32)))
        return off, sig[:t]

    def signature(self, i: int) -> np.ndarray:
        off, sig = self.download()
        return sig[off[i]:off[i + 1]].copy()

    def matrix(self, rows=None, cols=None, upper: bool = False, flags: int = 0):
        n = len(self)
        r0, r1 = rows or (0, n)
        c0, c1 = cols or (0, n)
        nr, nc = r1 - r0, c1 - c0
        common = np.full((nr, nc), -1, dtype=np.int32)
        D = np.full((nr, nc), np.nan, dtype=np.float64)
        fl = flags | (L.UPPER_TRIANGLE if upper else 0)
        L.check(L.lib.gdist_sketch_matrix(self.ctx.h, self.h, r0, r1, c0, c1, fl, common.ctypes.data,
                                          D.ctypes.data, max(nc, 1)))
        return common, D

    def closest(self, n: int, max_dist: float, rows: tuple[int, int] | None = None,
                cols: tuple[int, int] | None = None, flags: int = 0, keep_self: bool = False):
        """Exact nearest neighbours by sketch distance (gdist_closest; flags:
        SKETCH_JACCARD, EMPTY_NAN): the same result shape as KmerSets.closest, d
        bit-identical to matrix()'s D."""
        return self._closest(n, max_dist, rows, cols, L.METHOD_AUTO, flags, keep_self)

    def within(self, max_dist: float, rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
               upper: bool = False, method: int = L.METHOD_AUTO, flags: int = 0, keep_self: bool = False,
               capacity: int | None = None):
        """Every pair within a sketch distance (gdist_within; flags:
        SKETCH_JACCARD, EMPTY_NAN; method is ignored): as KmerSets.within, d
        bit-identical to matrix()'s D."""
        return self._within(max_dist, rows, cols, upper, L.METHOD_AUTO, flags, keep_self, capacity)

    def group_stats(self, labels, rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
                    upper: bool = True, method: int = L.METHOD_AUTO, flags: int = 0) -> GroupStats:
        """In-group / out-group summary of the sketch distances (gdist_group_stats;
        flags: SKETCH_JACCARD, EMPTY_NAN; method is ignored): as KmerSets.group_stats."""
        return self._group_stats(labels, rows, cols, upper, L.METHOD_AUTO, flags)

    def histogram(self, edges, labels=None, rows: tuple[int, int] | None = None,
                  cols: tuple[int, int] | None = None, upper: bool = True, method: int = L.METHOD_AUTO,
                  flags: int = 0) -> Histogram:
        """How the sketch distances are distributed (gdist_histogram; flags:
        SKETCH_JACCARD, EMPTY_NAN; method is ignored): as KmerSets.histogram."""
        return self._histogram(edges, labels, rows, cols, upper, L.METHOD_AUTO, flags)

    def quantiles(self, q, rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
                  upper: bool = True, method: int = L.METHOD_AUTO, flags: int = 0):
        """Exact order statistics of the sketch distances (flags: SKETCH_JACCARD,
        EMPTY_NAN; method is ignored): as KmerSets.quantiles."""
        return self._quantiles(q, rows, cols, upper, L.METHOD_AUTO, flags)

    # Query sketches against this resident sketch database (the reference's
    # find / mash: one getClosest per incoming genome). `queries` is a
    # SketchSets of the same width and kmer spec; this collection is only
    # read, nothing is built on it and nothing is copied. Each call gives, bit
    # for bit, what its one-collection twin gives on self.concat(queries) for
    # rows len(self) + rows x cols with keep_self. flags: SKETCH_JACCARD,
    # EMPTY_NAN (empty_nan=True adds the latter).
    def cross_matrix(self, queries: "SketchSets", rows: tuple[int, int] | None = None,
                     cols: tuple[int, int] | None = None, flags: int = 0, want_I: bool = True,
                     want_D: bool = True):
        """Common counts (matrix()'s `common`) and sketch distances of `queries`
        (rows) against this collection (cols) (gdist_cross_matrix)."""
        return self._cross_matrix(queries, rows, cols, flags, want_I, want_D)

    def cross_closest(self, queries: "SketchSets", n: int, max_dist: float, rows: tuple[int, int] | None = None,
                      cols: tuple[int, int] | None = None, flags: int = 0):
        """Exact nearest neighbours of `queries` among this collection by sketch
        distance (gdist_cross_closest): (idx, d, count) as KmerSets.cross_closest."""
        return self._cross_closest(queries, n, max_dist, rows, cols, flags)

    def cross_within(self, queries: "SketchSets", max_dist: float, rows: tuple[int, int] | None = None,
                     cols: tuple[int, int] | None = None, empty_nan: bool = False, capacity: int | None = None,
                     flags: int = 0):
        """Every (query, resident sketch) pair within a sketch distance
        (gdist_cross_within): CSR as KmerSets.cross_within."""
        return self._cross_within(queries, max_dist, rows, cols, flags | (L.EMPTY_NAN if empty_nan else 0), capacity)

    def cross_group_stats(self, queries: "SketchSets", qlabels, slabels, rows: tuple[int, int] | None = None,
                          cols: tuple[int, int] | None = None, empty_nan: bool = False,
                          flags: int = 0) -> GroupStats:
        """In-group / out-group summary of the sketch distances of `queries`
        against this collection (gdist_cross_group_stats): as KmerSets.cross_group_stats."""
        return self._cross_group_stats(queries, qlabels, slabels, rows, cols,
                                       flags | (L.EMPTY_NAN if empty_nan else 0))

    def cross_histogram(self, queries: "SketchSets", edges, qlabels=None, slabels=None,
                        rows: tuple[int, int] | None = None, cols: tuple[int, int] | None = None,
                        empty_nan: bool = False, flags: int = 0) -> Histogram:
        """How the sketch distances of `queries` against this collection are
        distributed (gdist_cross_histogram): as KmerSets.cross_histogram."""
        return self._cross_histogram(queries, edges, qlabels, slabels, rows, cols,
                                     flags | (L.EMPTY_NAN if empty_nan else 0))

    def pairs(self, rows, cols, other: "SketchSets | None" = None, flags: int = 0, want_common: bool = True,
              want_D: bool = True):
        """Sketch distances of a pair list (gdist_sketch_pairs): for every p the
        common count and sketch distance of signature rows[p] of this
        collection and signature cols[p] of `other` (default: this collection),
        in one device call: (common int32[P] | None, D float64[P] | None). Any
        order, repeats and (with one collection) i == j allowed; both are
        other.cross_matrix(self)'s cell (rows[p], cols[p]) bit for bit, with one
        collection matrix()'s. flags: SKETCH_JACCARD, EMPTY_NAN."""
        b = self if other is None else other
        return self._pairs(L.lib.gdist_sketch_pairs, (b.h,), rows, cols, (flags,), want_common, want_D)

    def row_query(self, q: int, cols: Iterable[int], mode: int = L.QUERY_ALL, t: float = 1.0,
                  other: "SketchSets | None" = None):
        """Signature q of this collection against signatures cols[] of `other`
        (default: this collection): one pair list with rows = [q] * len(cols),
        reduced on the host by the rules of gdist_row_query (reduce_row_query).
        ALL: the distances; ANY_LE: whether any is <= t; ARGMIN: (position in
        cols, distance), (-1, 1.0) when none is below 1.0."""
        cl = np.ascontiguousarray(np.fromiter(cols, dtype=np.int64))
        _, D = self.pairs(np.full(len(cl), q, dtype=np.int64), cl, other=other, want_common=False)
        return reduce_row_query(D, mode, t)

    def greedy_reps(self, max_dist: float, assign: bool = False, tie_rank: np.ndarray | None = None,
                    flags: int = 0):
        """Greedy representatives of the signatures on the device
        (gdist_sketch_greedy_reps), d the sketch distance matrix() returns under
        `flags` (SKETCH_JACCARD, EMPTY_NAN). Returns what KmerSets.greedy_reps
        returns: is_rep (int32[N]); with assign=True also (rep_of int64[N],
        rep_dist float64[N]), ties to the lowest tie_rank (default: index).
        Context.reps_info() reports the call."""
        n = len(self)
        is_rep = np.zeros(max(n, 1), dtype=np.int32)
        nreps = C.c_int64()
        rep_of = np.zeros(max(n, 1), dtype=np.int64) if assign else None
        rep_d = np.zeros(max(n, 1), dtype=np.float64) if assign else None
        tr = None
        if tie_rank is not None:
            tr = np.ascontiguousarray(tie_rank, dtype=np.int64)
            assert tr.shape == (n,)
        L.check(L.lib.gdist_sketch_greedy_reps(self.ctx.h, self.h, float(max_dist), int(flags),
                                               L.ptr(tr, C.c_int64) if tr is not None else None,
                                               L.ptr(is_rep, C.c_int32),
                                               L.ptr(rep_of, C.c_int64) if assign else None,
                                               L.ptr(rep_d, C.c_double) if assign else None, C.byref(nreps)))
        if assign:
            return is_rep[:n], rep_of[:n], rep_d[:n]
        return is_rep[:n]

    def matrix_device(self, d_common: int | None, d_D: int | None, ld: int, rows, cols, upper=False, flags=0):
        fl = flags | L.OUT_DEVICE | (L.UPPER_TRIANGLE if upper else 0)
        L.check(L.lib.gdist_sketch_matrix(self.ctx.h, self.h, rows[0], rows[1], cols[0], cols[1], fl, d_common,
                                          d_D, ld))


class LSHIndex:
    """LSHMemSeqHash over a SketchSets collection (gdist_lsh_build):
    getClosest(queries, n, maxDist) per query sketch."""

    def __init__(self, sketches: "SketchSets", stages: int, buckets: int, seed: int = 0x5EED):
        h = C.c_void_p()
        L.check(L.lib.gdist_lsh_build(sketches.ctx.h, sketches.h, int(stages), int(buckets), int(seed), C.byref(h)))
        self.ctx, self.h, self.sketches = sketches.ctx, h, sketches      # the index keeps its sketches alive
        self.ctx._handles.add(self)

    def free(self):
        if getattr(self, "h", None):
            L.lib.gdist_lsh_free(self.h)
            self.h = None

    def __del__(self):
        try:
            self.free()
        except Exception:
            pass

    def getClosest(self, queries: "SketchSets", n: int, max_dist: float) -> list[list[tuple[int, float]]]:
        """For each query: [(indexed set, distance)] nearest first, at most n, distance <= max_dist."""
        nq = len(queries)
        idx = np.zeros(max(nq * n, 1), dtype=np.int64)
        d = np.zeros(max(nq * n, 1), dtype=np.float64)
        cnt = np.zeros(max(nq, 1), dtype=np.int32)
        L.check(L.lib.gdist_lsh_closest(self.ctx.h, self.h, queries.h, int(n), float(max_dist),
                                        L.ptr(idx, C.c_int64), L.ptr(d, C.c_double), L.ptr(cnt, C.c_int32)))
        return [[(int(idx[q * n + r]), float(d[q * n + r])) for r in range(cnt[q])] for q in range(nq)]


def triangle_partition(n: int, nparts: int, align: int = 1) -> list[int]:
    """Row bounds with equal upper-triangle area per part."""
    b = np.zeros(nparts + 1, dtype=np.int64)
    L.check(L.lib.gdist_triangle_partition(n, nparts, align, L.ptr(b, C.c_int64)))
    return [int(x) for x in b]
