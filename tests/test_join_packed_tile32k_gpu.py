"""GPU parity of the 32 Ki-key tile of the pipelined packed partition kernel (TSQ_KNOB_DA_PARTITION = 4, k_da_partition2p<1024, ..>: one
workgroup per CU, 16-bit counter halves that reach 0x8000).  COUNT(*) on the packed route over a unique build side of 2^20 keys whose
range takes 20 or 27 bits (1024 partitions of 10-bit entries; 2048 partitions of 16-bit entries).  Every count is compared with numpy
on host copies of the keys and with the same pushes under TSQ_KNOB_DA_PARTITION = 2: batches around the tile (no whole tile, exactly
one, one and a tail, ...), more tiles than workgroups (the steady state of the pipeline), a batch whose rows all carry ONE key (a whole
tile in one partition: the 0x8000 edge of a counter half, and a run that leaves its region for the overflow list), and a batch in
which half the keys miss.  Without the knob a batch takes the tile from one 32 Ki-key tile per CU on: both sides of that size.
"""
import functools

import numpy as np
import pytest

from tinysql_amd import _abi as abi

from .test_join_packed_pipeline_gpu import _Join, _probe, _unique_build, _want

pytestmark = pytest.mark.gpu

T32 = 32 * 1024
BITS = [20, 27]


@functools.lru_cache(maxsize=None)
def _build(bits):
    bk, base, span = _unique_build(np.random.default_rng(bits), bits, step=1 << (bits - 20))
    assert len(bk) == 1 << 20
    bk.setflags(write=False)
    return bk, base, span


def _both(ctx, bits, batches):
    """the batches through one join per kernel; per kernel the counts after every push and the statistics after every push"""
    bk = _build(bits)[0]
    out = {}
    for part in (4, 2):
        with ctx.knobs(DA_PARTITION=part):
            j = _Join(ctx, bk)
            try:
                counts, stats = [], []
                for pk in batches:
                    j.push(pk)
                    counts.append(j.count())
                    stats.append(j.stats())
            finally:
                j.close()
        assert all(st.probe_route == abi.ROUTE_PACKED and st.packed_key_bits == bits and st.radix_bits == min(11, bits - 10) for st in stats)
        out[part] = (counts, stats)
    return out


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n_probe", [100, T32, T32 + 1, 2 * T32 + 5, 3 * T32 - 1])
def test_tile32k_edges(ctx, n_probe, bits):
    bk, base, span = _build(bits)
    rng = np.random.default_rng(n_probe + bits)
    pk = _probe(rng, bk, base, span, n_probe, 0.8)
    pk[:3] = [base - 1, base + span, -(1 << 62)]  # just below kmin, just above the range, far below
    got = _both(ctx, bits, [pk, pk])
    want = _want(bk, pk)
    assert got[4][0] == [want, 2 * want]
    assert got[2][0] == got[4][0]
    assert got[4][1][-1].radix_overflow_rows == 0  # the regions are sized for the real tile: a small batch stays in them


@pytest.mark.parametrize("bits", BITS)
def test_tile32k_more_tiles_than_workgroups(ctx, bits):
    # 300 tiles and a tail over at most one workgroup per CU: workgroups walk several tiles with the next tile's pieces in flight
    bk, base, span = _build(bits)
    rng = np.random.default_rng(300 + bits)
    pk = _probe(rng, bk, base, span, 300 * T32 + 77, 0.6)
    got = _both(ctx, bits, [pk])
    assert got[4][0] == [_want(bk, pk)]
    assert got[2][0] == got[4][0]


@pytest.mark.parametrize("bits", BITS)
@pytest.mark.parametrize("n_probe", [T32, 40000])
def test_tile32k_hot_key_fills_a_tile(ctx, n_probe, bits):
    # every row of the batch carries one build key: the partition's count is the whole tile (0x8000 in its counter half, the low or the
    # high one by the partition's parity), its run does not fit the region and leaves through the overflow list; 8 different keys
    bk = _build(bits)[0]
    keys = bk[np.random.default_rng(8).choice(len(bk), 8, replace=False)]
    batches = [np.full(n_probe, k, np.int64) for k in keys]
    got = _both(ctx, bits, batches)
    assert got[4][0] == [n_probe * (i + 1) for i in range(8)]
    assert got[2][0] == got[4][0]
    assert all(st.radix_overflow_rows > 0 for st in got[4][1])


@pytest.mark.parametrize("bits", BITS)
def test_tile32k_half_the_keys_miss(ctx, bits):
    bk, base, span = _build(bits)
    rng = np.random.default_rng(5 + bits)
    pk = _probe(rng, bk, base, span, 5 * T32 + 77, 0.5)
    got = _both(ctx, bits, [pk])
    want = _want(bk, pk)
    assert 0 < want < len(pk)
    assert got[4][0] == [want]
    assert got[2][0] == got[4][0]


@pytest.mark.parametrize("n_probe", [256 * T32 - 1, 256 * T32])
def test_default_takes_the_tile_from_one_tile_per_cu(ctx, n_probe):
    # 256 CUs: the last batch size that keeps the 16 Ki-key tiles and the first that takes the 32 Ki-key ones; same count either way
    bk, base, span = _build(27)
    rng = np.random.default_rng(n_probe)
    pk = _probe(rng, bk, base, span, n_probe, 0.7)
    want = _want(bk, pk)
    j = _Join(ctx, bk)
    try:
        j.push(pk)
        assert j.count() == want
        st = j.stats()
    finally:
        j.close()
    assert st.probe_route == abi.ROUTE_PACKED and st.radix_overflow_rows == 0
