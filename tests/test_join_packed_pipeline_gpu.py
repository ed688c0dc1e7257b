"""GPU parity of the COUNT(*) step of the packed-key route across its partition kernels and launch sequences: TSQ_KNOB_DA_PARTITION
2 (k_da_partition2) and 3 (k_da_partition2p: the next tile's key loads in flight while a tile is scanned, scattered and written out)
x TSQ_KNOB_DA_FUSED_STEP 0 (memsets + partition + probe + overflow kernel) and 1 (partition + probe: the probe kernel counts the
overflow list and leaves the cursors clean for the next batch).  Every combination must count what numpy counts on host copies of
the keys: ragged batches around the 16 Ki-key tile, a batch with more tiles than resident workgroups, key ranges of 13..27 bits at
hit ratios 1, 0.5 and 0, keys outside the range on both sides, a hot key that fills the overflow list before and after a batch
without overflow on the SAME join, batches of changing and of equal sizes on one join (with the kernels a step launches), a NULL
bitmap or selection flags between two plain pushes, and duplicate build keys.
"""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Chunk, Column

from . import gpu_helpers as G
from . import helpers as H

pytestmark = pytest.mark.gpu

FORCE = abi.RADIX_FORCE
T_TILE = 16 * 1024
PARTITION = [2, 3]
FUSED = [0, 1]


def _cfg(batch_rows=None):
    cfg = H.join_cfg([abi.I64, abi.I64], [abi.I64, abi.I64], [0], [0], abi.JOIN_INNER, 1)
    if batch_rows is not None:
        cfg.probe_batch_rows = batch_rows
    return cfg


def _chunk(keys, nn=None):
    return Chunk([Column(abi.I64, keys, nn), Column(abi.I64, np.arange(len(keys)))])


def _unique_build(rng, bits, base=-(1 << 36) + 77, step=8):
    # one key in every `step` cells (jittered), both ends of the range present: the range is exactly 2^bits cells; every key is negative
    span = 1 << bits
    bk = np.arange(0, span, step, dtype=np.int64) + rng.integers(0, step, span // step)
    bk[0], bk[-1] = 0, span - 1
    bk = np.unique(bk)
    rng.shuffle(bk)
    return base + bk, base, span


def _probe(rng, bk, base, span, n, hit):
    # `hit` of the rows take a build key; the others a key of the range that no build row has, or one below kmin / above the range
    pk = bk[rng.integers(0, len(bk), n)]
    miss = rng.random(n) >= hit
    m = int(miss.sum())
    if m:
        cand = base + rng.integers(-span // 16 - 5, span + span // 16 + 5, m)
        cand[np.isin(cand, bk)] = base - 7
        pk[miss] = cand
    return pk


def _want(bk, pk, keep=None):
    k = pk if keep is None else pk[keep]
    keys, cnts = np.unique(bk, return_counts=True)
    pos = np.searchsorted(keys, k)
    pos[pos == len(keys)] = 0
    return int(cnts[pos][keys[pos] == k].sum())


class _Join:
    """one COUNT(*) join on the packed route; probe batches are pushed as DEVICE columns (one da_probe step per push)"""

    def __init__(self, ctx, bk):
        self.ctx, self.lib = ctx, ctx.lib
        self.h = C.c_void_p()
        self.bufs = []
        _lib.check(self.lib.tsq_join_create(ctx.h, C.byref(_cfg()), C.byref(self.h)), ctx.h)
        _lib.check(self.lib.tsq_join_set_radix(self.h, FORCE), self.h)
        _lib.check(self.lib.tsq_join_set_key_packing(self.h, FORCE), self.h)
        G.push_chunked(self.lib.tsq_join_build_push, self.h, _chunk(bk), 1 << 24)
        _lib.check(self.lib.tsq_join_build_finish(self.h), self.h)
        _lib.check(self.lib.tsq_join_set_count_only(self.h, 1), self.h)

    def _dev(self, arr):
        arr = np.ascontiguousarray(arr)
        p = self.ctx.alloc(max(arr.nbytes, 16) + 64)
        self.bufs.append(p)
        self.ctx.h2d(p, arr)
        return p

    def push(self, pk, nn=None):
        n = len(pk)
        cols = (abi.Col * 2)()
        for i, arr in enumerate((pk.astype(np.int64), np.zeros(n, np.int64))):
            cols[i].data, cols[i].length, cols[i].elem_size, cols[i].type, cols[i].flags = self._dev(arr), n, 8, abi.I64, abi.COL_DEVICE
        if nn is not None:
            cols[0].null_bitmap = self._dev(np.packbits(nn.astype(np.uint8), bitorder="little"))
        _lib.check(self.lib.tsq_join_probe_push(self.h, cols, 2, n, None), self.h)

    def count(self):
        c = C.c_int64(0)
        _lib.check(self.lib.tsq_join_count(self.h, C.byref(c)), self.h)
        return c.value

    def stats(self):
        st = abi.Stats()
        _lib.check(self.lib.tsq_join_stats(self.h, C.byref(st)), self.h)
        return st

    def close(self):
        self.lib.tsq_join_destroy(self.h)
        for p in self.bufs:
            self.ctx.free(p)


def _count_once(ctx, bk, pk, part, fused):
    stats = []
    with ctx.knobs(DA_PARTITION=part, DA_FUSED_STEP=fused):
        got = G.run_join(ctx, _cfg(1 << 24), _chunk(bk), _chunk(pk), chunk_rows=1 << 24, count_only=True, radix=FORCE, packing=FORCE, stats_out=stats)
    assert stats[0].probe_route == abi.ROUTE_PACKED
    return got, stats[0]


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
@pytest.mark.parametrize("n_probe", [1, 63, T_TILE - 1, T_TILE, T_TILE + 1, 3 * T_TILE + 5])
def test_pipeline_ragged_batches(ctx, n_probe, part, fused):
    rng = np.random.default_rng(n_probe + 3 * part + fused)
    bk, base, span = _unique_build(rng, 20)
    pk = _probe(rng, bk, base, span, n_probe, 0.7)
    got, st = _count_once(ctx, bk, pk, part, fused)
    assert st.packed_key_bits == 20
    assert got == _want(bk, pk)


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
def test_pipeline_more_tiles_than_resident_workgroups(ctx, part, fused):
    # 2.5e7 rows = 1526 tiles over at most 512 workgroups: every workgroup runs the steady state of the pipeline, the last tile is partial
    rng = np.random.default_rng(77)
    bk, base, span = _unique_build(rng, 27, step=16)
    pk = _probe(rng, bk, base, span, 25_000_001, 0.6)
    want = _want(bk, pk)
    with ctx.knobs(DA_PARTITION=part, DA_FUSED_STEP=fused):
        j = _Join(ctx, bk)
        try:
            j.push(pk)
            assert j.count() == want
            j.push(pk)  # and once more through the store the first batch left behind
            assert j.count() == 2 * want
            st = j.stats()
        finally:
            j.close()
    assert st.probe_route == abi.ROUTE_PACKED and st.radix_bits == 11 and st.radix_overflow_rows == 0


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
@pytest.mark.parametrize("hit", [1.0, 0.5, 0.0])
@pytest.mark.parametrize("bits", [13, 16, 20, 27])
def test_pipeline_key_ranges_and_hit_ratios(ctx, bits, hit, part, fused):
    rng = np.random.default_rng(bits * 5 + int(hit * 10))
    bk, base, span = _unique_build(rng, bits, step=16 if bits >= 24 else 8)
    pk = _probe(rng, bk, base, span, 40 * T_TILE + 11, hit)
    pk[:3] = [base - 1, base + span, -(1 << 62)]  # just below kmin, just above the range, far below
    got, st = _count_once(ctx, bk, pk, part, fused)
    assert st.packed_key_bits == bits and st.radix_bits == min(11, bits - 10)
    assert got == _want(bk, pk)
    if hit == 0.0:
        assert got == 0


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
@pytest.mark.parametrize("hot_first", [True, False])
def test_pipeline_overflow_batch_next_to_a_plain_batch_on_one_join(ctx, hot_first, part, fused):
    # the overflow count and the valid_end marks of the hot batch must be gone when the next batch runs (and the reverse order)
    rng = np.random.default_rng(9 + hot_first)
    bk, base, span = _unique_build(rng, 20)
    n = 20 * T_TILE + 9
    plain = _probe(rng, bk, base, span, n, 0.8)
    hot = _probe(rng, bk, base, span, n, 0.8)
    hot[rng.random(n) < 0.5] = bk[5]
    order = [(hot, True), (plain, False), (hot, True)] if hot_first else [(plain, False), (hot, True), (plain, False)]
    with ctx.knobs(DA_PARTITION=part, DA_FUSED_STEP=fused):
        j = _Join(ctx, bk)
        try:
            total = 0
            for pk, is_hot in order:
                j.push(pk)
                total += _want(bk, pk)
                assert j.count() == total
                ovf = j.stats().radix_overflow_rows
                assert (ovf > 0) if is_hot else (ovf == 0)
        finally:
            j.close()


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
def test_pipeline_changing_then_equal_batch_sizes_and_launches(ctx, part, fused):
    rng = np.random.default_rng(41)
    bk, base, span = _unique_build(rng, 22)
    big, small = 60 * T_TILE + 123, 2 * T_TILE + 1
    sizes = [big, small, big, big, big, big]
    with ctx.knobs(DA_PARTITION=part, DA_FUSED_STEP=fused):
        j = _Join(ctx, bk)
        try:
            total, launches = 0, []
            for n in sizes:
                pk = _probe(rng, bk, base, span, n, 0.75)
                j.push(pk)
                total += _want(bk, pk)
                assert j.count() == total
                launches.append(j.stats().kernel_launches)
            st = j.stats()
        finally:
            j.close()
    assert st.probe_route == abi.ROUTE_PACKED and st.radix_batches == len(sizes)
    # kernels (not memsets) per step once the images exist: partition + probe, or partition + probe + overflow kernel
    assert [b - a for a, b in zip(launches[1:], launches[2:])] == [2 if fused else 3] * (len(sizes) - 2)


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
def test_pipeline_null_bitmap_between_plain_pushes(ctx, part, fused):
    # the FLAGS instantiation of k_da_partition2 runs in between: it must find the store clean and leave it usable
    rng = np.random.default_rng(31 + part)
    bk, base, span = _unique_build(rng, 22)
    n = 6 * T_TILE + 17
    p1, p2, p3 = (_probe(rng, bk, base, span, n, 0.75) for _ in range(3))
    nn2 = rng.random(n) > 0.1
    with ctx.knobs(DA_PARTITION=part, DA_FUSED_STEP=fused):
        j = _Join(ctx, bk)
        try:
            total = 0
            for pk, nn in ((p1, None), (p2, nn2), (p3, None), (p1, None)):
                j.push(pk, nn)
                total += _want(bk, pk, nn)
                assert j.count() == total
        finally:
            j.close()


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
def test_pipeline_selection_flags_between_plain_pushes(ctx, part, fused):
    # host chunks, the middle one with selected[] flags (a filtered-out row is treated like a NULL key)
    rng = np.random.default_rng(53 + part)
    bk, base, span = _unique_build(rng, 21)
    n = 5 * T_TILE + 64
    p1, p2, p3 = (_probe(rng, bk, base, span, n, 0.8) for _ in range(3))
    sel2 = (rng.random(n) > 0.3).astype(np.uint8)
    lib = ctx.lib
    with ctx.knobs(DA_PARTITION=part, DA_FUSED_STEP=fused):
        h = C.c_void_p()
        _lib.check(lib.tsq_join_create(ctx.h, C.byref(_cfg(n)), C.byref(h)), ctx.h)
        try:
            _lib.check(lib.tsq_join_set_radix(h, FORCE), h)
            _lib.check(lib.tsq_join_set_key_packing(h, FORCE), h)
            G.push_chunked(lib.tsq_join_build_push, h, _chunk(bk), 1 << 24)
            _lib.check(lib.tsq_join_build_finish(h), h)
            _lib.check(lib.tsq_join_set_count_only(h, 1), h)
            for pk, sel in ((p1, None), (p2, sel2), (p3, None)):
                keep = []
                part_chunk = _chunk(pk)
                cols = G.make_cols(part_chunk.columns, keep)
                _lib.check(lib.tsq_join_probe_push(h, cols, 2, n, None if sel is None else sel.ctypes.data_as(C.c_void_p)), h)
            _lib.check(lib.tsq_join_probe_finish(h), h)
            c = C.c_int64(0)
            _lib.check(lib.tsq_join_count(h, C.byref(c)), h)
            st = abi.Stats()
            _lib.check(lib.tsq_join_stats(h, C.byref(st)), h)
        finally:
            lib.tsq_join_destroy(h)
    assert st.probe_route == abi.ROUTE_PACKED
    assert c.value == _want(bk, p1) + _want(bk, p2, sel2 != 0) + _want(bk, p3)


@pytest.mark.parametrize("fused", FUSED)
@pytest.mark.parametrize("part", PARTITION)
def test_pipeline_duplicate_build_keys_byte_images(ctx, part, fused):
    rng = np.random.default_rng(5)
    bk, base, span = _unique_build(rng, 18)
    bk = np.concatenate([bk, bk[: len(bk) // 3], bk[:100]])  # up to three rows per key: the probe reads byte images, not bits
    rng.shuffle(bk)
    n = 7 * T_TILE + 3
    with ctx.knobs(DA_PARTITION=part, DA_FUSED_STEP=fused):
        j = _Join(ctx, bk)
        try:
            total = 0
            for _ in range(3):
                pk = _probe(rng, bk, base, span, n, 0.6)
                j.push(pk)
                total += _want(bk, pk)
                assert j.count() == total
        finally:
            j.close()
