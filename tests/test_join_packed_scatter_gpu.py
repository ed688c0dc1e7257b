"""GPU parity of the LDS side of the pipelined packed partition kernel (k_da_partition2p): the keys outside the build side's domain
(counted and scattered like any other key, into trash counters), the counters of a tile, the write-out.  COUNT(*) on the packed route over a unique build side of 4096 keys whose range takes
exactly 27 bits (2048 partitions, 2-byte entries) or 20 bits (1024 partitions), and 30 bits for the 4-byte entries; every expected
count is numpy's on host copies of the keys.  TSQ_KNOB_DA_PARTITION = 4 runs the 32 Ki-key tile of k_da_partition2p<1024, ..> at any
batch size, 3 the 16 Ki-key tile of the 512-thread instantiations.  With T the tile:
  row counts            T, T + 1, 2T - 1, 3T + 777 rows: the pipelined loop, the tail loop, and both
  share outside         full tiles in which half, all, or all but one of the keys lie outside the domain (below kmin, above kmax, far away)
  write-out groups      full tiles with 8192 k + r keys inside the domain, r in {0, 1, 1023, 1024, 7169}, k in {0, 1, 3}: the edges of a
                        write-out that takes eight positions per thread at a time (8 x 1024 per step of the workgroup), and of the
                        position-at-a-time loop's last round
  one partition         every key of a tile the same: one partition counts exactly T (0x8000 at T = 32 Ki: the most a 16-bit counter
                        half may reach without a carry); the run leaves its region through the overflow list
  hot key               a hot key in every other tile (its run overflows the region there) among keys outside the domain: the count includes
                        the overflow list, tiles with and without an overflowing run take their own write-out loops
"""
import functools

import numpy as np
import pytest

from tinysql_amd import _abi as abi

from .test_join_packed_pipeline_gpu import _Join, _unique_build, _want

pytestmark = pytest.mark.gpu

TILE = {4: 32 * 1024, 3: 16 * 1024}
# (key bits, TSQ_KNOB_DA_PARTITION): the 32 Ki-key tile takes 2-byte entries only; 30 bits = 4-byte entries, k_da_partition2p<512, .., uint32_t>
NARROW = [(27, 4), (20, 4), (27, 3)]
WIDE = (30, 3)


@functools.lru_cache(maxsize=None)
def _build(bits):
    bk, base, span = _unique_build(np.random.default_rng(bits), bits, step=1 << (bits - 12))
    assert len(bk) == 1 << 12
    bk.setflags(write=False)
    return bk, base, span


def _inside(rng, bits, n):
    """n keys of the domain: half of them build keys, the others any cell of the range (nearly all without a build row)"""
    bk, base, span = _build(bits)
    pk = bk[rng.integers(0, len(bk), n)]
    other = rng.random(n) < 0.5
    pk[other] = base + rng.integers(0, span, int(other.sum()))
    return pk


def _outside(rng, bits, n):
    """n keys outside [kmin, kmax]: just below, just above, far on both sides, the ends of int64"""
    _, base, span = _build(bits)
    d = rng.integers(1, span, n)
    pk = np.where(rng.random(n) < 0.5, base - d, base + span - 1 + d)
    far = rng.random(n) < 0.1
    pk[far] = rng.choice(np.array([np.iinfo(np.int64).min, np.iinfo(np.int64).max, base - 1, base + span, -(1 << 62), 1 << 62], np.int64), int(far.sum()))
    return pk


def _tile(rng, bits, t, n_inside):
    pk = np.concatenate([_inside(rng, bits, n_inside), _outside(rng, bits, t - n_inside)])
    rng.shuffle(pk)
    return pk


def _run(ctx, bits, part, batches):
    """counts and statistics after every push of one join under the knob"""
    bk = _build(bits)[0]
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
    assert all(st.probe_route == abi.ROUTE_PACKED and st.packed_key_bits == bits for st in stats)
    return counts, stats


def _wants(bits, batches):
    bk = _build(bits)[0]
    return list(np.cumsum([_want(bk, pk) for pk in batches]))


@pytest.mark.parametrize("bits,part", NARROW + [WIDE])
@pytest.mark.parametrize("shape", ["T", "T+1", "2T-1", "3T+777"])
def test_scatter_row_counts(ctx, shape, bits, part):
    t = TILE[part]
    n = {"T": t, "T+1": t + 1, "2T-1": 2 * t - 1, "3T+777": 3 * t + 777}[shape]
    rng = np.random.default_rng(n + bits)
    pk = np.concatenate([_tile(rng, bits, t, (3 * t) // 4) for _ in range(4)])[:n]
    counts, stats = _run(ctx, bits, part, [pk, pk])
    want = _wants(bits, [pk, pk])
    assert 0 < want[0] < n
    assert counts == want
    assert stats[-1].radix_overflow_rows == 0


@pytest.mark.parametrize("bits,part", NARROW)
@pytest.mark.parametrize("share", ["half", "all", "all but one"])
def test_scatter_keys_outside_the_domain_in_full_tiles(ctx, share, bits, part):
    # three full tiles and a tail of the same make; "all": no word of the tile is written out (total = 0)
    t = TILE[part]
    n_inside = {"half": t // 2, "all": 0, "all but one": 1}[share]
    rng = np.random.default_rng(len(share) + bits)
    bk = _build(bits)[0]
    tiles = [_tile(rng, bits, t, n_inside) for _ in range(3)] + [_tile(rng, bits, t, n_inside)[:777]]
    if share == "all but one":  # the one key inside the domain is a build key, at a different place in every tile
        for i, tl in enumerate(tiles[:3]):
            tl[:] = _outside(rng, bits, t)
            tl[(i * 12345 + 7) % t] = bk[i]
    pk = np.concatenate(tiles)
    counts, _ = _run(ctx, bits, part, [pk, pk[:2 * t]])
    want = _wants(bits, [pk, pk[:2 * t]])
    assert want[0] >= (3 if share == "all but one" else 0) and (share != "all" or want[-1] == 0)
    assert counts == want


@pytest.mark.parametrize("bits", [27, 20])
@pytest.mark.parametrize("k", [0, 1, 3])
def test_scatter_write_out_group_edges(ctx, k, bits):
    # one full tile per r, each with exactly 8192 k + r keys inside the domain; one workgroup per tile
    t = TILE[4]
    rng = np.random.default_rng(k + bits)
    pk = np.concatenate([_tile(rng, bits, t, 8192 * k + r) for r in (0, 1, 1023, 1024, 7169)])
    counts, stats = _run(ctx, bits, 4, [pk])
    assert counts == _wants(bits, [pk])
    assert stats[-1].radix_overflow_rows == 0


@pytest.mark.parametrize("bits,part", [(27, 4), (20, 4), (27, 3), (20, 3)])
def test_scatter_whole_tile_in_one_partition(ctx, bits, part):
    # every row of a batch carries one build key: its partition counts exactly T, the run leaves through the overflow list.  Keys of
    # partitions of both parities (the low and the high 16-bit half where two counters share a word): eight different keys
    t = TILE[part]
    bk = _build(bits)[0]
    keys = bk[np.random.default_rng(bits).choice(len(bk), 8, replace=False)]
    batches = [np.full(t, key, np.int64) for key in keys]
    counts, stats = _run(ctx, bits, part, batches)
    assert counts == [t * (i + 1) for i in range(8)]
    assert all(st.radix_overflow_rows > 0 for st in stats)


@pytest.mark.parametrize("bits,part", NARROW + [WIDE])
def test_scatter_hot_key_in_every_other_tile(ctx, bits, part):
    t = TILE[part]
    rng = np.random.default_rng(77 + bits)
    bk = _build(bits)[0]
    hot = bk[1234]
    tiles = []
    for i in range(6):
        tl = _tile(rng, bits, t, (4 * t) // 5)  # a fifth of every tile lies outside the domain
        if i % 2 == 0:
            tl[rng.random(t) < 0.6] = hot
        tiles.append(tl)
    pk = np.concatenate(tiles + [_tile(rng, bits, t, t // 2)[:4321]])
    counts, stats = _run(ctx, bits, part, [pk, pk])
    want = _wants(bits, [pk, pk])
    assert want[0] > int((pk == hot).sum()) > t
    assert counts == want
    assert stats[-1].radix_overflow_rows > 0
