"""GPU parity of the COUNT(*) probe of the packed-key route when the build side is UNIQUE: the probe then reads the bit form of
the byte images (TSQ_KNOB_DA_PROBE_BITS, csrc/tsq_join.hip da_probe), 8 KB per partition instead of 64 KB.  Every setting of the
knob (0 = byte images; n = bit images with n probe workgroups per CU) and both partition kernels must count what numpy counts:
ragged batch sizes around the 16 Ki-key tile, key ranges of 13..27 bits (log2 partitions 3..11), hit ratios of one and one half,
probe keys outside the range, a hot probe key that fills the overflow list, several pushes with a NULL bitmap between them,
several batches into one join, and a build side with duplicates (it keeps the byte images and counts multiplicities).
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
PROBE_BITS = [0, 1, 4, 8]  # 0: byte images
PARTITION = [0, 2]         # 0: the default kernel for 2-byte entries, 2: k_da_partition2


def _cfg(batch_rows=None):
    cfg = H.join_cfg([abi.I64, abi.I64], [abi.I64, abi.I64], [0], [0], abi.JOIN_INNER, 1)
    if batch_rows is not None:
        cfg.probe_batch_rows = batch_rows
    return cfg


def _chunk(keys, nn=None):
    return Chunk([Column(abi.I64, keys, nn), Column(abi.I64, np.arange(len(keys)))])


def _unique_build(rng, bits, base=-(1 << 36) + 77, step=8):
    # one key in every `step` cells (jittered), both ends of the range present: the range is exactly 2^bits cells
    span = 1 << bits
    bk = np.arange(0, span, step, dtype=np.int64) + rng.integers(0, step, span // step)
    bk[0], bk[-1] = 0, span - 1
    bk = np.unique(bk)
    rng.shuffle(bk)
    return base + bk, base, span


def _probe(rng, bk, base, span, n, hit):
    # `hit` of the rows take a build key; the others a key in the range that no build row has, or one outside the range
    pk = bk[rng.integers(0, len(bk), n)]
    miss = rng.random(n) >= hit
    m = int(miss.sum())
    if m:
        cand = base + rng.integers(-span // 16 - 5, span + span // 16 + 5, m)
        pk[miss] = cand
    return pk


def _want(bk, pk, pnn=None):
    k = pk if pnn is None else pk[pnn]
    keys, cnts = np.unique(bk, return_counts=True)
    pos = np.searchsorted(keys, k)
    pos[pos == len(keys)] = 0
    return int(cnts[pos][keys[pos] == k].sum())


def _count(ctx, build, probe, bits_knob, part_knob, cfg=None, chunk_rows=1 << 24):
    stats = []
    with ctx.knobs(DA_PROBE_BITS=bits_knob, DA_PARTITION=part_knob):
        got = G.run_join(ctx, cfg or _cfg(1 << 24), build, probe, chunk_rows=chunk_rows, count_only=True, radix=FORCE, packing=FORCE,
                         stats_out=stats)
    assert stats[0].probe_route == abi.ROUTE_PACKED
    return got, stats[0]


@pytest.mark.parametrize("part", PARTITION)
@pytest.mark.parametrize("bits_knob", PROBE_BITS)
@pytest.mark.parametrize("n_probe", [1, T_TILE - 1, T_TILE, T_TILE + 1, 3 * T_TILE + 5, 100 * T_TILE + 3])
def test_bit_probe_ragged_batches(ctx, n_probe, bits_knob, part):
    rng = np.random.default_rng(n_probe + 7 * bits_knob)
    bk, base, span = _unique_build(rng, 20)
    pk = _probe(rng, bk, base, span, n_probe, 0.7)
    got, st = _count(ctx, _chunk(bk), _chunk(pk), bits_knob, part)
    assert st.packed_key_bits == 20
    assert got == _want(bk, pk)


@pytest.mark.parametrize("bits_knob", PROBE_BITS)
@pytest.mark.parametrize("hit", [1.0, 0.5])
@pytest.mark.parametrize("bits", [13, 14, 17, 21, 24, 27])
def test_bit_probe_key_ranges(ctx, bits, hit, bits_knob):
    rng = np.random.default_rng(bits * 3 + int(hit * 10))
    bk, base, span = _unique_build(rng, bits, step=16 if bits >= 24 else 8)
    pk = _probe(rng, bk, base, span, 40 * T_TILE + 11, hit)
    got, st = _count(ctx, _chunk(bk), _chunk(pk), bits_knob, 0)
    assert st.packed_key_bits == bits
    assert st.radix_bits == min(11, bits - 10)
    assert got == _want(bk, pk)


@pytest.mark.parametrize("bits_knob", PROBE_BITS)
def test_bit_probe_1e7_rows(ctx, bits_knob):
    rng = np.random.default_rng(1234)
    bk, base, span = _unique_build(rng, 26, step=16)
    pk = _probe(rng, bk, base, span, 10_000_000, 0.5)
    got, _ = _count(ctx, _chunk(bk), _chunk(pk), bits_knob, 0)
    assert got == _want(bk, pk)


@pytest.mark.parametrize("part", PARTITION)
@pytest.mark.parametrize("bits_knob", PROBE_BITS)
def test_bit_probe_hot_key_fills_the_overflow_list(ctx, bits_knob, part):
    rng = np.random.default_rng(99)
    bk, base, span = _unique_build(rng, 20)
    pk = _probe(rng, bk, base, span, 20 * T_TILE + 9, 0.8)
    hot = rng.random(len(pk)) < 0.5
    pk[hot] = bk[5]
    got, st = _count(ctx, _chunk(bk), _chunk(pk), bits_knob, part)
    assert st.radix_overflow_rows > 0
    assert got == _want(bk, pk)


@pytest.mark.parametrize("bits_knob", PROBE_BITS)
def test_bit_probe_duplicate_build_keys_count_multiplicities(ctx, bits_knob):
    rng = np.random.default_rng(5)
    bk, base, span = _unique_build(rng, 18)
    bk = np.concatenate([bk, bk[: len(bk) // 3], bk[:100]])  # up to three rows per key
    rng.shuffle(bk)
    pk = _probe(rng, bk, base, span, 7 * T_TILE + 3, 0.6)
    got, _ = _count(ctx, _chunk(bk), _chunk(pk), bits_knob, 0)
    assert got == _want(bk, pk)


def _run_pushes(ctx, build, pushes, batch_rows):
    # one join, several probe pushes (each its own device batch): what the route keeps between batches must survive them
    lib = ctx.lib
    h = C.c_void_p()
    _lib.check(lib.tsq_join_create(ctx.h, C.byref(_cfg(batch_rows)), C.byref(h)), ctx.h)
    try:
        _lib.check(lib.tsq_join_set_radix(h, FORCE), h)
        _lib.check(lib.tsq_join_set_key_packing(h, FORCE), h)
        G.push_chunked(lib.tsq_join_build_push, h, build, 1 << 24)
        _lib.check(lib.tsq_join_build_finish(h), h)
        _lib.check(lib.tsq_join_set_count_only(h, 1), h)
        for part in pushes:
            keep = []
            cols = G.make_cols(part.columns, keep)
            _lib.check(lib.tsq_join_probe_push(h, cols, len(part.columns), part.NumRows(), None), h)
        _lib.check(lib.tsq_join_probe_finish(h), h)
        c = C.c_int64(0)
        _lib.check(lib.tsq_join_count(h, C.byref(c)), h)
        st = abi.Stats()
        _lib.check(lib.tsq_join_stats(h, C.byref(st)), h)
        return c.value, st
    finally:
        lib.tsq_join_destroy(h)


@pytest.mark.parametrize("part", PARTITION)
@pytest.mark.parametrize("bits_knob", PROBE_BITS)
def test_bit_probe_several_pushes_with_a_null_bitmap_between(ctx, bits_knob, part):
    rng = np.random.default_rng(31 + bits_knob)
    bk, base, span = _unique_build(rng, 22)
    n = 6 * T_TILE + 17
    p1, p2, p3 = (_probe(rng, bk, base, span, n, 0.75) for _ in range(3))
    nn2 = rng.random(n) > 0.1
    want = _want(bk, p1) + _want(bk, p2, nn2) + _want(bk, p3)
    with ctx.knobs(DA_PROBE_BITS=bits_knob, DA_PARTITION=part):
        got, st = _run_pushes(ctx, _chunk(bk), [_chunk(p1), _chunk(p2, nn2), _chunk(p3)], n)
    assert st.probe_route == abi.ROUTE_PACKED
    assert got == want


@pytest.mark.parametrize("bits_knob", PROBE_BITS)
def test_bit_probe_several_steps_in_a_row(ctx, bits_knob):
    rng = np.random.default_rng(8)
    bk, base, span = _unique_build(rng, 24)
    n = 50 * T_TILE + 1
    pk = _probe(rng, bk, base, span, n, 0.9)
    pk[: n // 10] = bk[3]  # and a hot key: the overflow list is used (and emptied) in every batch
    with ctx.knobs(DA_PROBE_BITS=bits_knob):
        got, st = _run_pushes(ctx, _chunk(bk), [_chunk(pk)] * 5, n)
    assert st.probe_route == abi.ROUTE_PACKED and st.radix_batches >= 5
    assert got == 5 * _want(bk, pk)
