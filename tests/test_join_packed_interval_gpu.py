"""COUNT(*) against a build side that fills its key interval (csrc/tsq_dajoin.h k_da_interval_count, csrc/tsq_join.hip da_probe_interval):
a unique build side with as many usable rows as kmax - kmin + 1 holds every key of [kmin, kmax], so a probe row joins iff its key is inside the
domain — one range test per key instead of partition + probe.  TSQ_KNOB_DA_INTERVAL: 1 (default) takes the route under AUTO key packing, 0
never, 2 also under FORCE (what these tests use on small build sides).  Every expected count is numpy's / Python's on host copies of the keys;
every interval case asserts packed_interval_batches == the batches pushed, every other case that it stays 0.  The last tests run the shapes of
the existing AUTO-packing tests once more with the knob at 0, so that the partitioned kernels stay covered at those shapes.
"""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Chunk, Column

from . import gpu_helpers as G
from . import helpers as H
from .test_join_radix_gpu import _device_count, _expected_hits

pytestmark = pytest.mark.gpu

FORCE = abi.RADIX_FORCE
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1


def _cfg(bt=abi.I64, pt=abi.I64):
    return H.join_cfg([pt], [bt], [0], [0], abi.JOIN_INNER, 1)


def _host_count(ctx, build, probe, cfg=None, packing=FORCE, selected=None, knobs=None):
    """one host push of the whole probe side (one device batch behind the staging buffers); (count, statistics)"""
    stats = []
    with ctx.knobs(**({"DA_INTERVAL": 2} if knobs is None else knobs)):
        got = G.run_join(ctx, cfg or _cfg(), build, probe, chunk_rows=1 << 24, count_only=True, radix=FORCE, packing=packing, selected=selected, stats_out=stats)
    return got, stats[0]


def _is_interval_batch(st, batches=1):
    return st.probe_route == abi.ROUTE_PACKED and st.packed_interval_batches == batches and st.radix_batches == batches and st.radix_overflow_rows == 0


class _DeviceJoin:
    """a COUNT(*) join handle over a host build side, probed with device batches that start at any row of a device column"""

    def __init__(self, ctx, bk, packing=FORCE):
        self.ctx, self.lib, self.bufs = ctx, ctx.lib, []
        self.h = C.c_void_p()
        cfg = _cfg()
        _lib.check(self.lib.tsq_join_create(ctx.h, C.byref(cfg), C.byref(self.h)), ctx.h)
        try:
            _lib.check(self.lib.tsq_join_set_radix(self.h, FORCE), self.h)
            if packing is not None:
                _lib.check(self.lib.tsq_join_set_key_packing(self.h, packing), self.h)
            G.push_chunked(self.lib.tsq_join_build_push, self.h, Chunk([Column(abi.I64, bk)]), 1 << 24)
            _lib.check(self.lib.tsq_join_build_finish(self.h), self.h)
            _lib.check(self.lib.tsq_join_set_count_only(self.h, 1), self.h)
        except Exception:
            self.close()
            raise

    def upload(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.alloc(arr.nbytes + 64)
        self.bufs.append(p)
        self.ctx.h2d(p, arr)
        return p

    def push(self, data_ptr, n, nulls_ptr=None):
        cols = (abi.Col * 1)()
        cols[0].data, cols[0].null_bitmap, cols[0].length, cols[0].elem_size, cols[0].type, cols[0].flags = data_ptr, nulls_ptr, n, 8, abi.I64, abi.COL_DEVICE
        _lib.check(self.lib.tsq_join_probe_push(self.h, cols, 1, n, None), self.h)

    def count(self):
        c = C.c_int64(0)
        _lib.check(self.lib.tsq_join_count(self.h, C.byref(c)), self.h)
        return c.value

    def stats(self):
        st = abi.Stats()
        _lib.check(self.lib.tsq_join_stats(self.h, C.byref(st)), self.h)
        return st

    def close(self):
        if self.h:
            self.lib.tsq_join_destroy(self.h)
            self.h = None
        for p in self.bufs:
            self.ctx.free(p)
        self.bufs = []


KMIN, NB = -1500, 4096


def _build_keys(rng, kmin=KMIN, n=NB):
    return (kmin + rng.permutation(n)).astype(np.int64)


# ------------------------------------------------------------------ device batches: row counts around the tile, the wave and the 16-byte unit
@pytest.mark.parametrize("odd_start", [0, 1], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("n", [1, 2, 3, 63, 64, 65, 255, 256, 257, 1023, 4097, 100_003])
def test_device_batch_row_counts_and_column_starts(ctx, n, odd_start):
    rng = np.random.default_rng(1000 * n + odd_start)
    pk = rng.integers(KMIN - NB // 2, KMIN + NB + NB // 2, n + 1).astype(np.int64)
    pk[odd_start], pk[odd_start + n - 1] = KMIN, KMIN + NB - 1  # the peeled first row and the last row are hits (both are one row for n = 1: kmax)
    rows = pk[odd_start:odd_start + n]
    want = int(np.count_nonzero((rows >= KMIN) & (rows < KMIN + NB)))
    with ctx.knobs(DA_INTERVAL=2):
        j = _DeviceJoin(ctx, _build_keys(rng))
        try:
            base = j.upload(pk)
            assert base % 16 == 0
            j.push(base + 8 * odd_start, n)
            got, st = j.count(), j.stats()
        finally:
            j.close()
    assert got == want and want >= 1
    assert _is_interval_batch(st) and st.packed_key_bits == 13


# ------------------------------------------------------------------ the edges of the domain
@pytest.mark.parametrize("n", [1, 2, 4096])
@pytest.mark.parametrize("kmin_of", [lambda n: -5000, lambda n: 0, lambda n: I64_MAX - n - 2, lambda n: I64_MAX - n + 1, lambda n: I64_MIN],
                         ids=["negative", "zero", "near_max", "kmax_is_max", "kmin_is_min"])
def test_domain_edges(ctx, n, kmin_of):
    kmin = kmin_of(n)
    kmax = kmin + n - 1
    rng = np.random.default_rng(n)
    cands = [k for k in (kmin - 1, kmin, kmax, kmax + 1, I64_MIN, I64_MAX, kmin + (1 << 63), kmin - (1 << 63), kmax + (1 << 63), kmax - (1 << 63)) if I64_MIN <= k <= I64_MAX]
    picks = [cands[i] for i in rng.integers(0, len(cands), 777)] + cands
    want = sum(1 for k in picks if kmin <= k <= kmax)  # Python integers: no wrapped arithmetic
    bk = np.array([kmin + int(i) for i in rng.permutation(n)], dtype=np.int64)
    got, st = _host_count(ctx, Chunk([Column(abi.I64, bk)]), Chunk([Column(abi.I64, np.array(picks, dtype=np.int64))]))
    assert got == want and want >= 2
    assert _is_interval_batch(st)


# ------------------------------------------------------------------ signedness: BIGINT / BIGINT UNSIGNED, an interval below 2^63
@pytest.mark.parametrize("bt,pt", [(abi.U64, abi.I64), (abi.I64, abi.U64), (abi.U64, abi.U64), (abi.I64, abi.I64)])
def test_signedness_pairings(ctx, bt, pt):
    rng = np.random.default_rng(17)
    kmin, n = 1000, 2000
    cells = (kmin + rng.permutation(n)).astype(np.uint64)  # the build side's 64-bit cells: below 2^63, the same value in both types
    pc = rng.integers(kmin - 500, kmin + n + 500, 40_000).astype(np.uint64)
    hi = rng.random(40_000) < 0.3
    pc[hi] += np.uint64(1 << 63)  # cells at or above 2^63: huge unsigned values / negative signed ones, some with low bits inside the range
    pc[:4] = [kmin, kmin + n - 1, (1 << 63) + kmin, (1 << 63) + kmin + n - 1]

    def value(cell, t):  # what the cell means in its column's type
        return cell - (1 << 64) if (t == abi.I64 and cell >= (1 << 63)) else cell

    bset = {value(int(c), bt) for c in cells}
    want = sum(1 for c in pc.tolist() if value(c, pt) in bset)
    build = Chunk([Column(bt, cells.view(np.int64) if bt == abi.I64 else cells)])
    probe = Chunk([Column(pt, pc.view(np.int64) if pt == abi.I64 else pc)])
    got, st = _host_count(ctx, build, probe, cfg=_cfg(bt, pt))
    assert got == want and 0 < want < 40_000 * 0.7
    assert _is_interval_batch(st)


# ------------------------------------------------------------------ NULL probe keys and selection flags around the bitmap's word edge
@pytest.mark.parametrize("n", [31, 32, 33, 64, 65])
@pytest.mark.parametrize("with_sel", [False, True], ids=["nulls", "nulls_and_sel"])
def test_null_probe_keys_and_selection_flags_host_push(ctx, n, with_sel):
    rng = np.random.default_rng(31 * n + with_sel)
    pk = rng.integers(KMIN - NB // 4, KMIN + NB + NB // 4, n).astype(np.int64)
    nn = rng.random(n) > 0.1
    nn[0], nn[n - 1] = False, True
    pk[n - 1] = KMIN
    sel = (rng.random(n) > 0.3).astype(np.uint8) if with_sel else None
    if with_sel:
        sel[n - 1] = 1
    usable = nn & (sel != 0 if with_sel else True)
    want = int(np.count_nonzero(usable & (pk >= KMIN) & (pk < KMIN + NB)))
    got, st = _host_count(ctx, Chunk([Column(abi.I64, _build_keys(rng))]), Chunk([Column(abi.I64, pk, nn)]), selected=sel)
    assert got == want and want >= 1
    assert _is_interval_batch(st)


@pytest.mark.parametrize("odd_start", [0, 1], ids=["aligned16", "aligned8"])
@pytest.mark.parametrize("n", [31, 32, 33, 64, 65, 4097])
def test_null_probe_keys_device_batch(ctx, n, odd_start):
    rng = np.random.default_rng(77 * n + odd_start)
    pk = rng.integers(KMIN - NB // 4, KMIN + NB + NB // 4, n + 1).astype(np.int64)
    nn = rng.random(n) > 0.1  # the bitmap of the BATCH: bit r = row r of the batch is NOT NULL
    nn[0], nn[n - 1] = True, False
    pk[odd_start], pk[odd_start + n - 1] = KMIN + 1, KMIN + 2  # a peeled first row that counts, a last row that is NULL
    rows = pk[odd_start:odd_start + n]
    want = int(np.count_nonzero(nn & (rows >= KMIN) & (rows < KMIN + NB)))
    with ctx.knobs(DA_INTERVAL=2):
        j = _DeviceJoin(ctx, _build_keys(rng))
        try:
            base, bm = j.upload(pk), j.upload(np.packbits(nn, bitorder="little"))
            j.push(base + 8 * odd_start, n, bm)
            got, st = j.count(), j.stats()
        finally:
            j.close()
    assert got == want and want >= 1
    assert _is_interval_batch(st)


# ------------------------------------------------------------------ several batches through one handle; which of them are timed
@pytest.mark.parametrize("interval_knob", [2, 0], ids=["interval", "partitioned"])
@pytest.mark.parametrize("batches,timing,timed", [(9, None, 2), (9, 1, 9), (9, 0, 0), (40, 1, 32)])
def test_batches_accumulate_and_are_timed_as_on_the_partitioned_route(ctx, batches, timing, timed, interval_knob):
    rng = np.random.default_rng(13)
    batch = 4096
    pk = rng.integers(KMIN - NB // 4, KMIN + NB + NB // 4, (batches, batch)).astype(np.int64)
    want = int(np.count_nonzero((pk >= KMIN) & (pk < KMIN + NB)))
    knobs = {"DA_INTERVAL": interval_knob}
    if timing is not None:
        knobs["JOIN_BATCH_TIMING"] = timing
    with ctx.knobs(**knobs):
        j = _DeviceJoin(ctx, _build_keys(rng))
        try:
            base = j.upload(pk)
            for b in range(batches):
                j.push(base + b * batch * 8, batch)
            got, st = j.count(), j.stats()
        finally:
            j.close()
    assert got == want
    assert st.probe_route == abi.ROUTE_PACKED and st.radix_batches == batches and st.radix_timed_batches == timed
    assert st.packed_interval_batches == (batches if interval_knob == 2 else 0)
    assert st.packed_key_bits == 13 and st.radix_overflow_rows == 0
    if timed == 0:
        assert st.partition_kernel_ms_sum == 0 and st.radix_probe_kernel_ms_sum == 0
    else:
        assert st.radix_probe_kernel_ms_sum > 0 and st.radix_probe_kernel_ms > 0 and st.probe_kernel_ms > 0 and st.partition_kernel_ms_sum >= 0


# ------------------------------------------------------------------ build sides that must NOT take the route
def _not_interval(ctx, build, probe, want, cfg=None):
    got, st = _host_count(ctx, build, probe, cfg=cfg)
    assert got == want
    assert st.probe_route == abi.ROUTE_PACKED and st.packed_interval_batches == 0 and st.radix_batches == 1


def test_one_key_missing(ctx):
    rng = np.random.default_rng(5)
    bk = np.delete(np.arange(NB, dtype=np.int64), 77)
    rng.shuffle(bk)
    pk = rng.integers(-100, NB + 100, 50_000).astype(np.int64)
    pk[:3] = [76, 77, 78]
    _not_interval(ctx, Chunk([Column(abi.I64, bk)]), Chunk([Column(abi.I64, pk)]), int(np.isin(pk, bk).sum()))


def test_one_key_missing_and_another_twice(ctx):
    # {0, 1, 1, 3}: as many usable rows as the range has cells — only uniqueness says no
    rng = np.random.default_rng(6)
    bk = np.array([0, 1, 1, 3], dtype=np.int64)
    pk = rng.integers(-2, 6, 10_000).astype(np.int64)
    want = int(np.count_nonzero(pk == 0) + 2 * np.count_nonzero(pk == 1) + np.count_nonzero(pk == 3))
    _not_interval(ctx, Chunk([Column(abi.I64, bk)]), Chunk([Column(abi.I64, pk)]), want)


def test_null_build_keys_that_leave_a_hole(ctx):
    rng = np.random.default_rng(7)
    bk = rng.permutation(NB).astype(np.int64)
    nn = ~np.isin(bk, [100, 2000])
    pk = rng.integers(-100, NB + 100, 50_000).astype(np.int64)
    pk[:4] = [99, 100, 2000, 2001]
    _not_interval(ctx, Chunk([Column(abi.I64, bk, nn)]), Chunk([Column(abi.I64, pk)]), int(np.isin(pk, bk[nn]).sum()))


def test_null_build_keys_outside_the_interval_do_not_matter(ctx):
    # (the other side of the previous case: NULL build rows are not usable rows, the remaining keys fill [0, NB))
    rng = np.random.default_rng(8)
    bk = np.concatenate([rng.permutation(NB), [5, 5, 9_999_999]]).astype(np.int64)
    nn = np.concatenate([np.ones(NB, bool), [False, False, False]])
    pk = rng.integers(-100, NB + 100, 50_000).astype(np.int64)
    got, st = _host_count(ctx, Chunk([Column(abi.I64, bk, nn)]), Chunk([Column(abi.I64, pk)]))
    assert got == int(np.count_nonzero((pk >= 0) & (pk < NB)))
    assert _is_interval_batch(st)


def test_two_key_columns(ctx):
    # every (a, b) of [0, 64) x [0, 64): the composite key fills its interval, but composed keys are out of scope
    rng = np.random.default_rng(9)
    k = rng.permutation(64 * 64)
    build = Chunk([Column(abi.I64, (k // 64).astype(np.int64)), Column(abi.I64, (k % 64).astype(np.int64))])
    pa, pb = rng.integers(-8, 72, 30_000).astype(np.int64), rng.integers(-8, 72, 30_000).astype(np.int64)
    want = int(np.count_nonzero((pa >= 0) & (pa < 64) & (pb >= 0) & (pb < 64)))
    cfg = H.join_cfg([abi.I64, abi.I64], [abi.I64, abi.I64], [0, 1], [0, 1], abi.JOIN_INNER, 1)
    _not_interval(ctx, build, Chunk([Column(abi.I64, pa), Column(abi.I64, pb)]), want, cfg=cfg)


# ------------------------------------------------------------------ the knob
@pytest.mark.parametrize("knobs,packing,taken", [({"DA_INTERVAL": 0}, FORCE, False), ({"DA_INTERVAL": 0, "DA_MIN_BUILD_ROWS": 1}, None, False), ({}, FORCE, False),
                                                 ({"DA_INTERVAL": 1}, FORCE, False), ({"DA_MIN_BUILD_ROWS": 1}, None, True), ({"DA_MIN_BUILD_ROWS": 1}, abi.RADIX_AUTO, True),
                                                 ({"DA_INTERVAL": 2}, FORCE, True), ({"DA_INTERVAL": 2, "DA_MIN_BUILD_ROWS": 1}, None, True)],
                         ids=["0_force", "0_auto", "default_force", "1_force", "default_auto", "default_auto_set", "2_force", "2_auto"])
def test_knob(ctx, knobs, packing, taken):
    rng = np.random.default_rng(21)
    pk = rng.integers(KMIN - NB, KMIN + 2 * NB, 60_000).astype(np.int64)
    got, st = _host_count(ctx, Chunk([Column(abi.I64, _build_keys(rng))]), Chunk([Column(abi.I64, pk)]), packing=packing, knobs=knobs)
    assert got == int(np.count_nonzero((pk >= KMIN) & (pk < KMIN + NB)))
    assert st.probe_route == abi.ROUTE_PACKED and st.radix_batches == 1
    assert st.packed_interval_batches == (1 if taken else 0)


# ------------------------------------------------------------------ re-coverage: the existing tests with AUTO packing and an interval build side take
# the range test now; the same shapes once more on the partitioned kernels (TSQ_KNOB_DA_INTERVAL = 0)
def test_partitioned_at_1e7_hit_ratio_half(ctx):
    # test_join_packed_gpu.py::test_packed_auto_at_1e7_hit_ratio_half
    rng = np.random.default_rng(9)
    n = 3 * (4 << 20)
    off = 5_000_000_000
    bk = off + rng.permutation(n).astype(np.int64)
    pk = off + rng.integers(0, 2 * n, n)
    cfg = H.join_cfg([abi.I64, abi.I64], [abi.I64, abi.I64], [0], [0], abi.JOIN_INNER, 1)
    build = Chunk([Column(abi.I64, bk), Column(abi.I64, np.arange(n))])
    probe = Chunk([Column(abi.I64, pk), Column(abi.I64, np.arange(n))])
    stats = []
    with ctx.knobs(DA_INTERVAL=0):
        got = G.run_join(ctx, cfg, build, probe, chunk_rows=1 << 24, count_only=True, stats_out=stats)
    assert got == int((pk < off + n).sum())
    assert stats[0].probe_route == abi.ROUTE_PACKED and stats[0].packed_key_bits == 24 and stats[0].radix_batches == 3 and stats[0].packed_interval_batches == 0


def test_partitioned_auto_on_large_device_batches(ctx):
    # test_join_radix_gpu.py::test_radix_auto_engages_on_large_batches_and_matches_direct_probe; and what the default does at this shape
    nb, npr, mod = 10_000_000, 30_000_000, 12_500_000
    want = _expected_hits(nb, npr, mod)
    with ctx.knobs(DA_INTERVAL=0, JOIN_BATCH_TIMING=1):  # (every batch timed: by default only every fourth one is)
        got, st = _device_count(ctx, nb, npr, mod, abi.RADIX_AUTO, steps=2)
    assert got == 2 * want and st.radix_batches == 2 and st.radix_overflow_rows == 0 and st.radix_bits >= 6
    assert st.probe_route == abi.ROUTE_PACKED and st.packed_interval_batches == 0 and st.partition_kernel_ms_sum > 0
    with ctx.knobs(JOIN_BATCH_TIMING=1):
        got, st = _device_count(ctx, nb, npr, mod, abi.RADIX_AUTO, steps=2)
    assert got == 2 * want and st.radix_batches == 2 and st.radix_overflow_rows == 0 and st.radix_bits >= 6
    assert st.probe_route == abi.ROUTE_PACKED and st.packed_interval_batches == 2 and st.radix_timed_batches == 2 and st.radix_probe_kernel_ms_sum > 0


def test_partitioned_full_size_1e8_by_1e8(ctx):
    # test_join_radix_gpu.py::test_radix_full_size_1e8_by_1e8_property (its first half: the route and the count)
    n = 100_000_000
    with ctx.knobs(DA_INTERVAL=0):
        got, st = _device_count(ctx, n, n, n, abi.RADIX_AUTO)
    assert got == n and st.radix_batches == 1 and st.radix_bits >= 10 and st.radix_overflow_rows == 0
    assert st.probe_route == abi.ROUTE_PACKED and st.table_buckets == 0 and st.packed_interval_batches == 0
