"""GPU: GROUP BY / SELECT DISTINCT over more than four key columns (tsq_agg_create_keys) through executor.HashAggExec (host chunks of
1024 rows) and gpu_pipeline.GpuHashAggExec (device chunks).

Expected result: the oracle's hash_agg GROUP BY the REFERENCE group id (one key, tests/groupid_ref.py) over the same rows + the id
column.  Group order is unspecified, so results are compared as multisets: the id column travels through both sides as an ordinary
argument (FIRST_ROW(rid): any row of a group carries the same value) and lines the groups up — a group split or merged on the GPU
shows as a missing or repeated id.  Integers, counts, MIN / MAX and strings are bit-exact; SUM / AVG(double) within SURVEY §8(d)'s
reordering bound 2 n_g 2^-53 sum|v_i| per group; FIRST_ROW(key column) through the group-key encoding (any row of the group may serve)."""
import ctypes as C

import numpy as np
import pytest

from tests import groupid_ref as R
from tests import helpers as H
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Chunk, Column, StrColumn, concat, out_buffers
from tinysql_amd.executor import AggFuncDesc, HashAggExec, MockDataSource
from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceTableScan, GpuHashAggExec

pytestmark = pytest.mark.gpu


def make_input(rows, n_keys, colset, keyset):
    """key columns 0..n_keys-1, then v_i64, v_f64, s_val, s_grp, rid"""
    keys = R.make_keys(rows, n_keys, colset, keyset)
    rid = R.np_ids(keys)
    rng = np.random.default_rng(rows + 31 * n_keys)
    v_i64 = Column(abi.I64, rng.integers(-(1 << 40), 1 << 40, rows), rng.random(rows) >= 0.1)
    v_f64 = Column(abi.F64, (rng.random(rows) - 0.5) * 1e6, rng.random(rows) >= 0.1)
    s_val = StrColumn([None if x % 11 == 0 else b"v%d" % (x % 977) for x in rng.integers(0, 1 << 30, rows).tolist()])
    s_grp = StrColumn([None if g % 5 == 0 else (b"g%d" % g) * (g % 4 + 1) for g in rid.tolist()])
    return Chunk(keys + [v_i64, v_f64, s_val, s_grp, Column(abi.I64, rid.astype(np.int64))]), rid


def plan_a(n_keys, types, key_firstrows=True):
    """(descriptors, kind per output column); kind: 'x' exact, 's' / 'a' SUM / AVG of a double, 'k' a key column, 'r' the id"""
    vi, vf, sv, sg, rid = n_keys, n_keys + 1, n_keys + 2, n_keys + 3, n_keys + 4
    d = [AggFuncDesc(abi.AGG_COUNT, -1), AggFuncDesc(abi.AGG_COUNT, vi, abi.I64)]
    kinds = ["x", "x"]
    for f in (abi.AGG_SUM, abi.AGG_AVG, abi.AGG_MAX, abi.AGG_MIN):
        d.append(AggFuncDesc(f, vi, abi.I64))
        kinds.append("x")
    for f, k in ((abi.AGG_SUM, "s"), (abi.AGG_AVG, "a"), (abi.AGG_MAX, "x"), (abi.AGG_MIN, "x")):
        d.append(AggFuncDesc(f, vf, abi.F64))
        kinds.append(k)
    d += [AggFuncDesc(abi.AGG_MAX, sv, abi.BYTES), AggFuncDesc(abi.AGG_MIN, sv, abi.BYTES), AggFuncDesc(abi.AGG_FIRSTROW, sg, abi.BYTES),
          AggFuncDesc(abi.AGG_FIRSTROW, rid, abi.I64)]
    kinds += ["x", "x", "x", "r"]
    for k in (0, n_keys - 1) if key_firstrows else ():
        d.append(AggFuncDesc(abi.AGG_FIRSTROW, k, types[k]))
        kinds.append("k")
    return d, kinds


def plan_keys(n_keys, types, with_rid):
    """FIRST_ROW of every key column (SELECT DISTINCT), + the id when the schema has room for it"""
    d = [AggFuncDesc(abi.AGG_FIRSTROW, k, types[k]) for k in range(n_keys)]
    kinds = ["k"] * n_keys
    if with_rid:
        d.append(AggFuncDesc(abi.AGG_FIRSTROW, len(types) - 1, abi.I64))
        kinds.append("r")
    return d, kinds


def run_host(ctx, chunk, group_by, descs, stats_out=None, est_groups=0):
    exe = HashAggExec(ctx, MockDataSource(ctx, chunk, 1024), group_by, descs, est_groups=est_groups)
    exe.Open()
    out = []
    try:
        while True:
            chk = exe.Next()
            if chk.NumRows() == 0:
                break
            out.append(chk)
        if stats_out is not None:
            st = abi.Stats()
            _lib.check(ctx.lib.tsq_agg_stats(exe.h, C.byref(st)), exe.h)
            stats_out.append(st)
    finally:
        exe.Close()
    return concat(out, exe.Schema())


def run_device(ctx, chunk, group_by, descs, stats_out=None, batch_rows=1 << 24):
    table = DeviceChunk.from_host(ctx, chunk)
    exe = GpuHashAggExec(ctx, DeviceTableScan(ctx, table, batch_rows), group_by, descs, pull_rows=1 << 16)
    exe.Open()
    out = []
    try:
        while True:
            chk = exe.Next()
            if chk.NumRows() == 0:
                break
            out.append(chk.to_host())
        if stats_out is not None:
            st = abi.Stats()
            _lib.check(ctx.lib.tsq_agg_stats(exe.h, C.byref(st)), exe.h)
            stats_out.append(st)
    finally:
        exe.Close()
        table.free()
    return concat(out, exe.Schema())


def oracle_by_rid(orc, chunk, descs):
    types = chunk.types()
    rid = len(types) - 1
    aggs = [(f.func, f.arg_col, f.arg_type, f.mode, f.arg_col2) for f in descs]
    return orc.hash_agg(H.agg_cfg(types, [rid], aggs), chunk, 4, 4)


def _nn(col):
    return np.ones(len(col), bool) if col.notnull is None else col.notnull


def assert_same_groups(got, want, kinds, chunk, rid, n_keys):
    """both results lined up by the id column, then column by column"""
    r = kinds.index("r")
    assert got.NumRows() == want.NumRows()
    if got.NumRows() == 0:
        return
    go, wo = np.argsort(got.columns[r].data, kind="stable"), np.argsort(want.columns[r].data, kind="stable")
    ids = want.columns[r].data[wo]
    assert np.array_equal(got.columns[r].data[go], ids) and len(np.unique(ids)) == len(ids), "the groups differ (split or merged keys)"
    vf = chunk.columns[n_keys + 1]
    absv = np.where(_nn(vf), np.abs(vf.data), 0.0)
    n_g = np.bincount(rid.astype(np.int64), minlength=int(ids.max()) + 1)
    bound = 2.0 * n_g * 2.0 ** -53 * np.bincount(rid.astype(np.int64), weights=absv, minlength=len(n_g))
    cnt = np.maximum(1, np.bincount(rid.astype(np.int64), weights=_nn(vf).astype(np.float64), minlength=len(n_g)))
    for c, kind in enumerate(kinds):
        g, w = R.take(got.columns[c], go), R.take(want.columns[c], wo)
        assert g.tp == w.tp, c
        assert np.array_equal(_nn(g), _nn(w)), "NULLs of output column %d" % c
        if kind in ("s", "a"):
            tol = bound[ids] / (cnt[ids] if kind == "a" else 1.0)
            bad = np.abs(g.data - w.data) > tol
            assert not bad.any(), "output column %d: %r vs %r (bound %r)" % (c, g.data[bad][:3], w.data[bad][:3], tol[bad][:3])
        elif kind == "k" and g.tp != abi.BYTES:  # through the group-key encoding: any row of the group may have served
            (fg, ig), (fw, iw) = R._images(g), R._images(w)
            assert np.array_equal(fg, fw) and np.array_equal(ig, iw), "key output column %d" % c
        elif g.tp == abi.BYTES:
            assert g.values() == w.values(), "output column %d" % c
        else:
            assert g.data.tobytes() == w.data.tobytes(), "output column %d" % c


def _cases_a():
    out = []
    for i, cs in enumerate(R.COLSETS):
        for j, ks in enumerate(R.KEYSETS):
            out.append((37, 5 if (i + j) % 2 else 7, cs, ks))
        out.append((1, 5, cs, "one"))
        out.append((5000, 7 if i % 2 else 5, cs, R.KEYSETS[i % 5]))
    out += [(5000, 5, "mixed", "distinct"), (5000, 7, "nulls5", "perm"), (200001, 5, "i64", "distinct"), (200001, 7, "nulls5", "sqrt"),
            (200001, 7, "bytes_mid", "lastcol")]
    return sorted(set(out))


@pytest.mark.parametrize("rows,n_keys,colset,keyset", _cases_a())
def test_functions_over_many_keys_host_and_device(ctx, orc, rows, n_keys, colset, keyset):
    chunk, rid = make_input(rows, n_keys, colset, keyset)
    descs, kinds = plan_a(n_keys, chunk.types())
    want = oracle_by_rid(orc, chunk, descs)
    hs, ds = [], []
    got_h = run_host(ctx, chunk, list(range(n_keys)), descs, hs)
    got_d = run_device(ctx, chunk, list(range(n_keys)), descs, ds)
    assert_same_groups(got_h, want, kinds, chunk, rid, n_keys)
    assert_same_groups(got_d, want, kinds, chunk, rid, n_keys)  # (so host and device path give the same multiset)
    assert hs[0].build_partitioned == 5 and ds[0].build_partitioned == 5
    assert hs[0].probe_rows == rows and ds[0].probe_rows == rows and hs[0].out_rows == want.NumRows()


@pytest.mark.parametrize("rows,colset,keyset", [(37, "mixed", "perm"), (37, "nulls5", "sqrt"), (5000, "bytes_last", "sqrt"), (5000, "nulls5", "lastcol"),
                                                (5000, "allnull", "distinct"), (200001, "mixed", "sqrt")])
@pytest.mark.parametrize("n_keys", [6, 16])
def test_select_distinct(ctx, orc, rows, colset, keyset, n_keys):
    keys = R.make_keys(rows, n_keys, colset, keyset)
    rid = R.np_ids(keys)
    with_rid = n_keys < 16
    chunk = Chunk(keys + ([Column(abi.I64, rid.astype(np.int64))] if with_rid else []))
    descs, kinds = plan_keys(n_keys, chunk.types(), with_rid)
    first = R.first_rows(rid)
    for got in (run_host(ctx, chunk, list(range(n_keys)), descs), run_device(ctx, chunk, list(range(n_keys)), descs)):
        assert got.NumRows() == len(first)
        # the distinct rows of the reference, as sets of rows of cell images
        want_rows = sorted(zip(*[[(int(a), int(b)) for a, b in zip(*R._images(R.take(k, first)))] if k.tp != abi.BYTES else R.take(k, first).values() for k in keys]), key=repr)
        got_rows = sorted(zip(*[[(int(a), int(b)) for a, b in zip(*R._images(c))] if c.tp != abi.BYTES else c.values() for c in got.columns[:n_keys]]), key=repr)
        assert got_rows == want_rows
        if with_rid:
            assert sorted(got.columns[n_keys].data.tolist()) == list(range(len(first)))


def test_host_batches_smaller_than_the_input(ctx, orc):
    chunk, rid = make_input(20000, 7, "nulls5", "sqrt")
    descs, kinds = plan_a(7, chunk.types())
    want = oracle_by_rid(orc, chunk, descs)
    with ctx.knobs(AGG_BATCH_ROWS=4096):  # five device batches: ids of known keys stay, new keys continue the numbering
        got = run_host(ctx, chunk, list(range(7)), descs)
    assert_same_groups(got, want, kinds, chunk, rid, 7)
    got = run_device(ctx, chunk, list(range(7)), descs, batch_rows=4096)  # five device chunks
    assert_same_groups(got, want, kinds, chunk, rid, 7)


@pytest.mark.parametrize("rows,n_keys,colset,keyset", [(37, 5, "mixed", "sqrt"), (5000, 7, "nulls5", "sqrt"), (5000, 5, "bytes_last", "distinct")])
def test_plan_without_a_first_row_of_a_key(ctx, orc, rows, n_keys, colset, keyset):
    # (every function goes to the child aggregate as it is; with FIRST_ROW(key column) the dictionary serves that column)
    chunk, rid = make_input(rows, n_keys, colset, keyset)
    descs, kinds = plan_a(n_keys, chunk.types(), key_firstrows=False)
    want = oracle_by_rid(orc, chunk, descs)
    st = []
    assert_same_groups(run_host(ctx, chunk, list(range(n_keys)), descs, st), want, kinds, chunk, rid, n_keys)
    assert_same_groups(run_device(ctx, chunk, list(range(n_keys)), descs, st), want, kinds, chunk, rid, n_keys)
    assert [x.build_partitioned for x in st] == [5, 5]


def test_collisions_are_counted_in_the_statistics(ctx, orc):
    chunk, rid = make_input(5000, 5, "i64", "sqrt")
    descs, kinds = plan_a(5, chunk.types())
    want = oracle_by_rid(orc, chunk, descs)
    with ctx.knobs(GROUPID_TAG_BITS=4):
        st = []
        got = run_device(ctx, chunk, list(range(5)), descs, st)
    assert_same_groups(got, want, kinds, chunk, rid, 5)
    assert st[0].build_partitioned == 5 and st[0].build_handed_back_rows > 0


def test_partial1_then_final_over_six_keys(ctx, orc):
    n_keys, rows = 6, 5000
    chunk, rid = make_input(rows, n_keys, "nulls5", "sqrt")
    t = chunk.types()
    vi, vf, ridc = n_keys, n_keys + 1, n_keys + 4
    keys = list(range(n_keys))

    def funcs(mode):
        return ([AggFuncDesc(abi.AGG_COUNT, -1, abi.I64, mode), AggFuncDesc(abi.AGG_SUM, vi, abi.I64, mode), AggFuncDesc(abi.AGG_AVG, vf, abi.F64, mode),
                 AggFuncDesc(abi.AGG_FIRSTROW, ridc, abi.I64, mode)] + [AggFuncDesc(abi.AGG_FIRSTROW, k, t[k], mode) for k in keys])

    complete = run_device(ctx, chunk, keys, funcs(abi.MODE_COMPLETE))
    # two partial aggregates over the halves of the input, then one FINAL aggregate that groups the partial columns by the same 6 keys
    parts = [run_host(ctx, chunk.slice(0, 2600), keys, funcs(abi.MODE_PARTIAL1)), run_device(ctx, chunk.slice(2600, rows), keys, funcs(abi.MODE_PARTIAL1))]
    ptypes = parts[0].types()  # count, sum, (avg count, avg sum), rid, k0..k5
    partial = concat(parts, ptypes)
    pk = list(range(5, 5 + n_keys))
    fin = ([AggFuncDesc(abi.AGG_COUNT, 0, abi.I64, abi.MODE_FINAL), AggFuncDesc(abi.AGG_SUM, 1, abi.I64, abi.MODE_FINAL),
            AggFuncDesc(abi.AGG_AVG, 2, abi.F64, abi.MODE_FINAL, 3), AggFuncDesc(abi.AGG_FIRSTROW, 4, abi.I64, abi.MODE_FINAL)] +
           [AggFuncDesc(abi.AGG_FIRSTROW, c, ptypes[c], abi.MODE_FINAL) for c in pk])
    kinds = ["x", "x", "a", "r"] + ["k"] * n_keys
    st = []
    final = run_host(ctx, partial, pk, fin, st)
    assert st[0].build_partitioned == 5
    assert_same_groups(final, complete, kinds, chunk, rid, n_keys)
    want = oracle_by_rid(orc, chunk, funcs(abi.MODE_COMPLETE))
    assert_same_groups(complete, want, kinds, chunk, rid, n_keys)


def test_empty_input_gives_zero_rows(ctx):
    types = [abi.I64] * 6
    empty = Chunk([Column(abi.I64, np.zeros(0, np.int64)) for _ in types])
    descs = [AggFuncDesc(abi.AGG_COUNT, -1)] + [AggFuncDesc(abi.AGG_FIRSTROW, k, abi.I64) for k in range(6)]
    assert run_host(ctx, empty, list(range(6)), descs).NumRows() == 0
    # a device scan without a chunk: the operator is created over the six-column schema and sees no row
    exe = GpuHashAggExec(ctx, _EmptyScan(ctx, types), list(range(6)), descs)
    exe.Open()
    try:
        assert exe.Next().NumRows() == 0
    finally:
        exe.Close()
    # ... and straight through the C-ABI: finish without a push, then a pull
    cfg = H.agg_cfg(types, [], [(abi.AGG_COUNT, -1, abi.I64)])
    h = C.c_void_p()
    _lib.check(ctx.lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), (C.c_int32 * 6)(*range(6)), (C.c_int32 * 6)(*types), 6, C.byref(h)), ctx.h)
    try:
        _lib.check(ctx.lib.tsq_agg_finish(h), h)
        keep = []
        out, _ = out_buffers([abi.I64], 1024, keep)
        n, eos = C.c_int64(-1), C.c_int32(0)
        _lib.check(ctx.lib.tsq_agg_pull(h, out, 1, 1024, C.byref(n), C.byref(eos)), h)
        assert n.value == 0 and eos.value == 1
    finally:
        ctx.lib.tsq_agg_destroy(h)


class _EmptyScan(DeviceTableScan):
    def __init__(self, ctx, types):
        super().__init__(ctx, DeviceChunk([], 0))
        self.types = list(types)


@pytest.mark.parametrize("n_keys", [1, 2, 3, 4])
def test_up_to_four_keys_are_exactly_tsq_agg_create(ctx, orc, n_keys):
    keys = R.make_keys(5000, n_keys, "mixed", "sqrt")
    v = Column(abi.I64, np.arange(5000) % 91 - 40)
    chunk = Chunk(keys + [v])
    types = chunk.types()
    aggs = [(abi.AGG_COUNT, -1, abi.I64), (abi.AGG_SUM, n_keys, abi.I64), (abi.AGG_MIN, n_keys, abi.I64)] + [(abi.AGG_FIRSTROW, k, types[k]) for k in range(n_keys)]
    out_types = [abi.I64] * 3 + types[:n_keys]
    from tests import gpu_helpers as G
    st_a = []
    want = G.run_agg(ctx, H.agg_cfg(types, list(range(n_keys)), aggs), chunk, out_types, stats_out=st_a)
    cfg = H.agg_cfg(types, [], aggs)
    lib, h = ctx.lib, C.c_void_p()
    kc, kt = (C.c_int32 * n_keys)(*range(n_keys)), (C.c_int32 * n_keys)(*types[:n_keys])
    _lib.check(lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), kc, kt, n_keys, C.byref(h)), ctx.h)
    try:
        G.push_chunked(lib.tsq_agg_push, h, chunk, 1024)
        _lib.check(lib.tsq_agg_finish(h), h)
        st = abi.Stats()
        _lib.check(lib.tsq_agg_stats(h, C.byref(st)), h)
        assert st.build_partitioned != 5 and st.build_partitioned == st_a[0].build_partitioned
        got = []
        while True:
            keep = []
            out, bufs = G.out_buffers(out_types, 1024, keep)
            n, eos = C.c_int64(0), C.c_int32(0)
            _lib.check(lib.tsq_agg_pull(h, out, len(out_types), 1024, C.byref(n), C.byref(eos)), h)
            if n.value == 0:
                break
            got.append(G.chunk_from_buffers(out_types, bufs, n.value))
        # (FIRST_ROW of a double key may come from any row of the group: -0.0 and +0.0 share one, so both sides lose the sign of zero)
        def unsigned_zero(chunk):
            return Chunk([Column(c.tp, c.data + 0.0, c.notnull) if c.tp in (abi.F32, abi.F64) else c for c in chunk.columns])
        assert H.rows_equal_unordered(unsigned_zero(concat(got, out_types)), unsigned_zero(want))
    finally:
        lib.tsq_agg_destroy(h)


def test_refusals(ctx):
    lib = ctx.lib
    # 16 distinct argument columns and 5 keys: the group id has no input column left
    types = [abi.I64] * 16
    cfg = H.agg_cfg(types, [], [(abi.AGG_SUM, c, abi.I64) for c in range(16)])
    kc, kt = (C.c_int32 * 5)(0, 1, 2, 3, 4), (C.c_int32 * 5)(*[abi.I64] * 5)
    h = C.c_void_p()
    assert lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), kc, kt, 5, C.byref(h)) == abi.ERR_UNSUPPORTED and not h.value
    # 15 distinct argument columns fit
    cfg = H.agg_cfg(types, [], [(abi.AGG_SUM, c, abi.I64) for c in range(15)])
    _lib.check(lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), kc, kt, 5, C.byref(h)), ctx.h)
    try:
        assert lib.tsq_agg_set_stream(h, 1) == abi.ERR_UNSUPPORTED  # StreamAgg over wide keys is out of scope
        assert lib.tsq_agg_set_fast(h, abi.AGGFAST_OFF) == abi.OK
        n = C.c_int64(-1)
        assert lib.tsq_agg_num_groups(h, C.byref(n)) == abi.OK and n.value == 0
        assert lib.tsq_agg_cancel(h) == abi.OK
        assert lib.tsq_agg_finish(h) == abi.ERR_CANCELLED
    finally:
        lib.tsq_agg_destroy(h)
    # keys in the cfg AND in the call, no keys, too many keys, a key type that is not the column's
    bad = H.agg_cfg(types, [0], [(abi.AGG_COUNT, -1, abi.I64)])
    assert lib.tsq_agg_create_keys(ctx.h, C.byref(bad), kc, kt, 5, C.byref(h)) == abi.ERR_INVALID
    cfg = H.agg_cfg(types, [], [(abi.AGG_COUNT, -1, abi.I64)])
    assert lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), kc, kt, 0, C.byref(h)) == abi.ERR_INVALID
    k17, t17 = (C.c_int32 * 17)(*[i % 16 for i in range(17)]), (C.c_int32 * 17)(*[abi.I64] * 17)
    assert lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), k17, t17, 17, C.byref(h)) == abi.ERR_UNSUPPORTED
    tbad = (C.c_int32 * 5)(abi.I64, abi.F64, abi.I64, abi.I64, abi.I64)
    assert lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), kc, tbad, 5, C.byref(h)) == abi.ERR_INVALID
