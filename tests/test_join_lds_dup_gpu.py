"""GPU parity of the materialising packed join with the build side in LDS and DUPLICATE build keys (round 9, csrc/tsq_damat_dup.h): the
two partition levels of the unique variant, then k_dmd_count sizes every final partition's OUTPUT rows and k_dmd_emit keeps the build
rows as runs per distinct key in LDS and assigns its writes by output row, so one probe row makes up to 255 rows (the byte cell's
maximum: executor/join_test.go:101-104, 134-160 are duplicate-key joins).  Inner / left outer / right outer, NULL keys and NULL payload
cells on both sides, probe keys outside the build side's range, OtherConditions and outer-side filters (the outer cases need the "first
candidate of its outer row" flags), selected[], several key columns, several device batches, and every way out of the variant —
everything is compared with the oracle; the variant is asserted through tsq_stats.packed_lds_dup, TSQ_KNOB_DA_LDS_DUP = 2 takes it for
any build side and TSQ_KNOB_DA_LDS_BUILD forces every S."""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column, concat

from . import gpu_helpers as G
from . import helpers as H

pytestmark = pytest.mark.gpu
FORCE = abi.RADIX_FORCE


def _pay(rng, n, c, null_pay):
    tp = (abi.I64, abi.F64, abi.U64)[c % 3]
    if tp == abi.F64:
        data = rng.random(n)
    elif tp == abi.U64:
        data = rng.integers(0, 1 << 63, n).astype(np.uint64)
    else:
        data = rng.integers(-(1 << 40), 1 << 40, n)
    return Column(tp, data, (rng.random(n) > null_pay) if c % 2 else None)


def _max_multiplicity(*key_cols):
    """the most build rows any key has (rows with a NULL key cell are never inserted: hash_table.go:161-163)"""
    ok = np.ones(len(key_cols[0]), bool)
    for c in key_cols:
        if c.notnull is not None:
            ok &= c.notnull
    if not ok.any():
        return 0
    keys = np.stack([np.asarray(c.data)[ok] for c in key_cols], axis=1)
    return int(np.unique(keys, axis=0, return_counts=True)[1].max())


def _dup_build(rng, n, lo, hi, ncols, null_key=0.02, null_pay=0.1):
    b = Chunk([Column(abi.I64, rng.integers(lo, hi, n), (rng.random(n) > null_key) if null_key else None)] + [_pay(rng, n, c, null_pay) for c in range(1, ncols)])
    assert 1 < _max_multiplicity(b.columns[0]) <= 255
    return b


def _probe(rng, n, lo, hi, ncols, null_key=0.03, null_pay=0.1):
    return Chunk([Column(abi.I64, rng.integers(lo, hi, n), rng.random(n) > null_key)] + [_pay(rng, n, c + 1, null_pay) for c in range(1, ncols)])


def _rows(ctx, cfg, build, probe, want_dup=1, chunk_rows=1 << 22, selected=None, lds_build=1, dup=2, packed=True):
    stats = []
    with ctx.knobs(DA_LDS_DUP=dup, DA_LDS_BUILD=lds_build):
        got = G.run_join(ctx, cfg, build, probe, chunk_rows=chunk_rows, pull_rows=8192, radix=FORCE, packing=FORCE, stats_out=stats, selected=selected)
    st = stats[0]
    if packed:
        assert st.probe_route == abi.ROUTE_PACKED, (st.probe_route, st.radix_batches)
    assert st.packed_lds_dup == want_dup, (st.packed_lds_dup, st.packed_lds_bits, st.radix_bits)
    if want_dup:
        assert st.packed_lds_bits > 0
    return got, st


def _same(got, want):
    assert got.NumRows() == want.NumRows() and H.rows_equal_unordered(got, want)


JOINS = [(abi.JOIN_INNER, 1), (abi.JOIN_INNER, 0), (abi.JOIN_LEFT_OUTER, 1), (abi.JOIN_RIGHT_OUTER, 0)]


@pytest.mark.parametrize("jt,inner", JOINS)
@pytest.mark.parametrize("n_probe,np_cols,nb_cols,knob", [(1, 1, 1, 1), (64, 2, 2, 2), (4097, 4, 6, 3), (60_001, 8, 8, 4), (33_333, 2, 1, 5)])
def test_lds_dup_vs_oracle(ctx, orc, jt, inner, n_probe, np_cols, nb_cols, knob):
    rng = np.random.default_rng(13 * n_probe + jt + inner)
    bside = _dup_build(rng, 6000, -900, 1000, nb_cols)     # about 3 rows per key, some keys of the range absent; NULL keys and payload cells
    pside = _probe(rng, n_probe, -1100, 1200, np_cols)     # misses inside the range and on both sides of it; NULL keys
    left, right = (pside, bside) if inner == 1 else (bside, pside)
    cfg = H.join_cfg(left.types(), right.types(), [0], [0], jt, inner)
    want = orc.hash_join(cfg, bside, pside)
    got, st = _rows(ctx, cfg, bside, pside, lds_build=knob)
    _same(got, want)
    if knob >= 2:
        assert st.packed_lds_bits == st.radix_bits + (knob - 2)


def test_lds_dup_host_chunks_of_1024_rows(ctx, orc):
    rng = np.random.default_rng(3)
    bside = _dup_build(rng, 6000, -900, 1000, 3)
    pside = _probe(rng, 20_001, -1100, 1200, 3)
    cfg = H.join_cfg(pside.types(), bside.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1)
    got, _ = _rows(ctx, cfg, bside, pside, chunk_rows=1024, lds_build=3)  # host chunks of tidb_max_chunk_size rows reach the same batch
    _same(got, orc.hash_join(cfg, bside, pside))


def _edge_sides(rng, a_rows):
    # build side: key A has a_rows rows, key B one, key C two, the others are random (1 .. 4 rows per key)
    A, B, Cc = 700, 701, 702
    others = rng.integers(0, 690, 5000)
    keys = np.concatenate([np.full(a_rows, A), [B], [Cc, Cc], others])
    keys = keys[rng.permutation(len(keys))]
    nb = len(keys)
    bside = Chunk([Column(abi.I64, keys), _pay(rng, nb, 1, 0.1), _pay(rng, nb, 2, 0.0)])
    # probe side: A 3000 times in a row (765 000 output rows from one run of probe rows: the expansions cross many tiles and odd bases);
    # before and after it B, C, hits and misses inside the range, and keys beyond the range (misses that never reach a partition: the
    # run must fit its level-1 region, which the batch's size decides)
    n_near = 3000
    near = rng.choice(np.concatenate([[B, Cc, 695, 703], rng.integers(0, 690, 60)]), 2 * n_near)
    far = rng.integers(5000, 9000, 134_000)
    keys_p = np.concatenate([far[:60_000], near[:n_near], np.full(3000, A), near[n_near:], far[60_000:]])
    n = len(keys_p)
    pside = Chunk([Column(abi.I64, keys_p, rng.random(n) > 0.01), _pay(rng, n, 1, 0.1)])
    return bside, pside


@pytest.mark.parametrize("jt", [abi.JOIN_INNER, abi.JOIN_LEFT_OUTER])
def test_lds_dup_multiplicity_255(ctx, orc, jt):
    rng = np.random.default_rng(43 + jt)
    bside, pside = _edge_sides(rng, 255)
    assert _max_multiplicity(bside.columns[0]) == 255
    cfg = H.join_cfg(pside.types(), bside.types(), [0], [0], jt, 1)
    want = orc.hash_join(cfg, bside, pside)
    got, _ = _rows(ctx, cfg, bside, pside)
    _same(got, want)


def test_lds_dup_multiplicity_256_is_refused_as_before(ctx, orc):
    rng = np.random.default_rng(47)
    bside, pside = _edge_sides(rng, 256)  # a byte cell cannot count 256 rows: the packed routes hand the join back
    assert _max_multiplicity(bside.columns[0]) == 256
    pside = pside.slice(55_000, 75_000)
    cfg = H.join_cfg(pside.types(), bside.types(), [0], [0], abi.JOIN_INNER, 1)
    want = orc.hash_join(cfg, bside, pside)
    got, st = _rows(ctx, cfg, bside, pside, want_dup=0, packed=False)
    assert st.probe_route != abi.ROUTE_PACKED
    _same(got, want)


@pytest.mark.parametrize("jt,inner", [(abi.JOIN_INNER, 1), (abi.JOIN_RIGHT_OUTER, 0)])
def test_lds_dup_no_payload(ctx, orc, jt, inner):
    rng = np.random.default_rng(53 + jt)
    bside = _dup_build(rng, 5000, 0, 1500, 1)
    pside = _probe(rng, 40_001, -100, 1600, 1)
    left, right = (pside, bside) if inner == 1 else (bside, pside)
    cfg = H.join_cfg(left.types(), right.types(), [0], [0], jt, inner)
    got, _ = _rows(ctx, cfg, bside, pside, lds_build=3)
    _same(got, orc.hash_join(cfg, bside, pside))


@pytest.mark.parametrize("jt,inner,filtered", [(abi.JOIN_INNER, 1, False), (abi.JOIN_LEFT_OUTER, 1, False), (abi.JOIN_RIGHT_OUTER, 0, False),
                                                (abi.JOIN_LEFT_OUTER, 1, True), (abi.JOIN_RIGHT_OUTER, 0, True)])
def test_lds_dup_other_conditions_and_outer_filter(ctx, orc, jt, inner, filtered):
    # OtherConditions over the joined rows (joiner.go:155-167, 351-378): an outer row ALL of whose candidates fail becomes one padded row
    # (274-281) — the candidates of an outer row are consecutive output rows and the emit kernel flags the first; the outer-side filter
    # of an outer join (join.go:328-345)
    rng = np.random.default_rng(59 + jt + 7 * filtered)
    n, nb = 60_000, 6000
    bside = Chunk([Column(abi.I64, rng.integers(0, 2000, nb), rng.random(nb) > 0.02), Column(abi.I64, rng.integers(-50, 50, nb), rng.random(nb) > 0.1)])
    assert 1 < _max_multiplicity(bside.columns[0]) <= 255
    pside = Chunk([Column(abi.I64, rng.integers(-200, 2200, n), rng.random(n) > 0.03), Column(abi.I64, rng.integers(-50, 50, n), rng.random(n) > 0.1)])
    left, right = (pside, bside) if inner == 1 else (bside, pside)
    keep = []
    conds = [E.ScalarFunction("gt", E.ScalarFunction("plus", E.Column(1, abi.I64), E.Column(3, abi.I64)), E.Constant(0))]
    filt = [E.ScalarFunction("lt", E.Column(1, abi.I64), E.Constant(30))] if filtered else ()  # (over the outer side's own row)
    cfg = H.join_cfg(left.types(), right.types(), [0], [0], jt, inner, conds, filt, keep)
    got, _ = _rows(ctx, cfg, bside, pside, lds_build=4)
    _same(got, orc.hash_join(cfg, bside, pside))


def test_lds_dup_selected_flags(ctx, orc):
    # an externally evaluated outer-side filter (tsq_join_probe_push's selected[]): a row with flag 0 behaves like a row with a NULL key
    rng = np.random.default_rng(61)
    n = 50_000
    bside = _dup_build(rng, 4000, 0, 1500, 2)
    pside = _probe(rng, n, -100, 1600, 3)
    sel = (rng.random(n) > 0.3).astype(np.uint8)
    for jt in (abi.JOIN_INNER, abi.JOIN_LEFT_OUTER):
        cfg = H.join_cfg(pside.types(), bside.types(), [0], [0], jt, 1)
        want = orc.hash_join(cfg, bside, pside, selected=sel)
        got, _ = _rows(ctx, cfg, bside, pside, selected=sel, lds_build=3)
        _same(got, want)


def test_lds_dup_two_key_columns(ctx, orc):
    # several integer key columns ride the packed routes as one composite column (k_da_compose): the key columns travel like payload
    rng = np.random.default_rng(67)
    nb, n = 6000, 60_000
    pairs = rng.integers(0, 50 * 40, nb)  # 3 build rows per composite key
    bside = Chunk([Column(abi.I64, pairs // 40 - 30, rng.random(nb) > 0.02), Column(abi.I64, pairs % 40 + 1000), _pay(rng, nb, 1, 0.1)])
    assert 1 < _max_multiplicity(bside.columns[0], bside.columns[1]) <= 255
    pside = Chunk([Column(abi.I64, rng.integers(-35, 25, n), rng.random(n) > 0.03), Column(abi.I64, rng.integers(995, 1045, n), rng.random(n) > 0.03), _pay(rng, n, 2, 0.1)])
    for jt in (abi.JOIN_INNER, abi.JOIN_LEFT_OUTER):
        cfg = H.join_cfg(pside.types(), bside.types(), [0, 1], [0, 1], jt, 1)
        got, _ = _rows(ctx, cfg, bside, pside, lds_build=4)
        _same(got, orc.hash_join(cfg, bside, pside))


def test_lds_dup_three_device_batches_prepare_the_build_side_once(ctx, orc):
    rng = np.random.default_rng(71)
    batch = 30_016  # (a multiple of 64 rows)
    bside = _dup_build(rng, 6000, 0, 2000, 3)
    pside = _probe(rng, 3 * batch, -100, 2100, 2)
    cfg = H.join_cfg(pside.types(), bside.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1, probe_batch_rows=batch)
    want = orc.hash_join(cfg, bside, pside)
    lib = ctx.lib
    out_types = pside.types() + bside.types()
    got, per_batch = [], []
    h = C.c_void_p()
    with ctx.knobs(DA_LDS_DUP=2, DA_LDS_BUILD=3):
        _lib.check(lib.tsq_join_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
        try:
            _lib.check(lib.tsq_join_set_radix(h, FORCE), h)
            _lib.check(lib.tsq_join_set_key_packing(h, FORCE), h)
            keep = []
            _lib.check(lib.tsq_join_build_push(h, G.make_cols(bside.columns, keep), len(bside.columns), bside.NumRows()), h)
            _lib.check(lib.tsq_join_build_finish(h), h)

            def pull_all():
                while True:
                    keep = []
                    out, bufs = G.out_buffers(out_types, 8192, keep, None)
                    nr, eos = C.c_int64(0), C.c_int32(0)
                    _lib.check(lib.tsq_join_pull(h, out, len(out_types), 8192, C.byref(nr), C.byref(eos)), h)
                    if nr.value == 0:
                        return
                    got.append(G.chunk_from_buffers(out_types, bufs, nr.value))

            for b in range(3):
                part = pside.slice(b * batch, (b + 1) * batch)
                keep = []
                _lib.check(lib.tsq_join_probe_push(h, G.make_cols(part.columns, keep), len(part.columns), batch, None), h)
                pull_all()
                st = abi.Stats()
                _lib.check(lib.tsq_join_stats(h, C.byref(st)), h)
                per_batch.append((st.radix_batches, st.packed_lds_dup, st.probe_route, st.packed_build_ms))
            _lib.check(lib.tsq_join_probe_finish(h), h)
            pull_all()
        finally:
            lib.tsq_join_destroy(h)
    assert [p[:3] for p in per_batch] == [(1, 1, abi.ROUTE_PACKED), (2, 1, abi.ROUTE_PACKED), (3, 1, abi.ROUTE_PACKED)], per_batch
    assert per_batch[0][3] > 0 and per_batch[1][3] == per_batch[0][3] and per_batch[2][3] == per_batch[0][3], per_batch
    _same(concat(got, out_types), want)


@pytest.mark.parametrize("jt", [abi.JOIN_INNER, abi.JOIN_LEFT_OUTER])
def test_lds_dup_skewed_probe_keys_fall_back(ctx, orc, jt):
    # a hot probe key overflows its level-1 region: the batch is taken by the sorted-columns variant (its overflow list), the next,
    # evenly spread batch of the same join by the LDS variant again
    rng = np.random.default_rng(73 + jt)
    build = _dup_build(rng, 6000, 0, 3000, 2, null_key=0.0)
    n = 70_000
    hot = Chunk([Column(abi.I64, rng.choice(np.array([5, 5, 5, 101, 2900, 77, -3, 50_000], dtype=np.int64), n), rng.random(n) > 0.02), _pay(rng, n, 1, 0.1)])
    cfg = H.join_cfg(hot.types(), build.types(), [0], [0], jt, 1)
    got, st = _rows(ctx, cfg, build, hot, want_dup=0)
    _same(got, orc.hash_join(cfg, build, hot))
    assert st.radix_overflow_rows > 0
    even = _probe(rng, n, -100, 3100, 2)
    nn = lambda c: c.notnull if c.notnull is not None else np.ones(len(c), bool)  # noqa: E731
    both = Chunk([Column(c0.tp, np.concatenate([c0.data, c1.data]), np.concatenate([nn(c0), nn(c1)])) for c0, c1 in zip(hot.columns, even.columns)])
    cfg2 = H.join_cfg(both.types(), build.types(), [0], [0], jt, 1, probe_batch_rows=70_016)  # (rounded up to 64 rows)
    got, st = _rows(ctx, cfg2, build, both, want_dup=1, chunk_rows=70_016)  # two device batches: the last one is (almost) even
    _same(got, orc.hash_join(cfg2, build, both))


def test_lds_dup_build_side_too_large_for_lds(ctx, orc):
    # 60 000 rows x 8 columns over a 13-bit key range with S = 1: 8 partitions of ~7500 rows x 56 B of payload
    rng = np.random.default_rng(79)
    bside = _dup_build(rng, 60_000, 0, 8000, 8)
    pside = _probe(rng, 30_000, -100, 8100, 2)
    cfg = H.join_cfg(pside.types(), bside.types(), [0], [0], abi.JOIN_INNER, 1)
    got, _ = _rows(ctx, cfg, bside, pside, want_dup=0, lds_build=2)
    _same(got, orc.hash_join(cfg, bside, pside))


def test_lds_dup_knobs(ctx, orc):
    rng = np.random.default_rng(83)
    pside = _probe(rng, 30_000, -1100, 1200, 2)
    b3000, b6000 = _dup_build(rng, 3000, -900, 1000, 2), _dup_build(rng, 6000, -900, 1000, 2)
    cfg = H.join_cfg(pside.types(), b6000.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1)
    want3000, want6000 = orc.hash_join(cfg, b3000, pside), orc.hash_join(cfg, b6000, pside)
    got, _ = _rows(ctx, cfg, b6000, pside, want_dup=0, dup=0)           # never
    _same(got, want6000)
    got, _ = _rows(ctx, cfg, b3000, pside, want_dup=0, dup=4096)        # fewer build rows than the threshold
    _same(got, want3000)
    got, _ = _rows(ctx, cfg, b6000, pside, want_dup=1, dup=4096)        # ... at least as many
    _same(got, want6000)
    got, st = _rows(ctx, cfg, b6000, pside, want_dup=0, lds_build=0)    # both LDS variants off
    _same(got, want6000)
    assert st.packed_lds_bits == 0


def test_lds_dup_leaves_the_unique_variant_alone(ctx, orc):
    rng = np.random.default_rng(89)
    keys = rng.permutation(np.arange(-900, 1000))[:1500]
    uniq = Chunk([Column(abi.I64, keys, rng.random(1500) > 0.02), _pay(rng, 1500, 1, 0.1)])
    assert _max_multiplicity(uniq.columns[0]) == 1
    pside = _probe(rng, 30_000, -1100, 1200, 2)
    cfg = H.join_cfg(pside.types(), uniq.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1)
    got, st = _rows(ctx, cfg, uniq, pside, want_dup=0)
    assert st.packed_lds_bits > 0
    _same(got, orc.hash_join(cfg, uniq, pside))
