"""GPU: every handle kind and every stateless entry point gives back what it took.  One context with a 1 GiB arena (tsq_ctx_reserve): a
kind is created, fed a tiny input, drained and closed, and the arena's `used` is 0 again while its `peak` shows that the kind's buffers
did come from the slab (the slab is reserved anew before each kind, so the peak is that kind's own).  The owners are C++ objects whose
destructors release their members (tsq_internal.h: DevBuf, PinnedBuf, DevEvent); a member that a destroy function forgot used to leak
silently.  The routes are forced the way their own tests force them, at the smallest sizes at which those tests engage them; results
are checked by those tests, here only lightly.  The failure paths that need no HIP error end at used == 0 as well."""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column, StrColumn, make_cols, out_buffers

from . import gpu_helpers as G
from . import helpers as H

pytestmark = pytest.mark.gpu

FORCE, OFF = abi.RADIX_FORCE, abi.RADIX_OFF
ARENA = 1 << 30
T2 = [abi.I64, abi.I64]


@pytest.fixture(scope="module")
def actx():
    ctx = _lib.Context(0)
    ctx.reserve(ARENA)
    yield ctx
    ctx.close()


def _table(rng, n, keys, null_keys=0.03):
    return Chunk([Column(abi.I64, rng.integers(0, keys, n), rng.random(n) > null_keys), Column(abi.I64, rng.integers(-99, 99, n))])


def _words(n, mod, every):
    return StrColumn([None if i % every == 0 else b"w%d" % (i % mod) for i in range(n)])


# ---------------------------------------------------------------- joins
def join_table_route(ctx, orc):
    rng = np.random.default_rng(1)
    build, probe = _table(rng, 3000, 800), _table(rng, 5000, 900)
    keep = []
    conds = [E.ScalarFunction("gt", E.ScalarFunction("plus", E.Column(1, abi.I64), E.Column(3, abi.I64)), E.Constant(0))]
    cfg = H.join_cfg(T2, T2, [0], [0], abi.JOIN_LEFT_OUTER, 1, conds, (), keep)
    assert G.run_join(ctx, cfg, build, probe, chunk_rows=4096).NumRows() == orc.hash_join(cfg, build, probe).NumRows()


def _count_join(ctx, orc, packing, route):
    rng = np.random.default_rng(2)
    build, probe = _table(rng, 3000, 900, 0.1), _table(rng, 16385, 1000, 0.1)
    cfg = H.join_cfg(T2, T2, [0], [0], abi.JOIN_INNER, 1)
    stats = []
    got = G.run_join(ctx, cfg, build, probe, chunk_rows=1 << 22, count_only=True, radix=FORCE, packing=packing, stats_out=stats)
    assert got == orc.hash_join(cfg, build, probe).NumRows() and stats[0].radix_batches >= 1
    if route is not None:
        assert stats[0].probe_route == route


def join_radix_route(ctx, orc):
    _count_join(ctx, orc, OFF, None)


def join_packed_count(ctx, orc):
    _count_join(ctx, orc, FORCE, abi.ROUTE_PACKED)


def join_packed_rows(ctx, orc):
    """the materialising packed route: a unique build side (in LDS), then duplicate build keys"""
    rng = np.random.default_rng(3)
    probe = _table(rng, 5000, 1200)
    uniq = Chunk([Column(abi.I64, rng.permutation(1000)[:700]), Column(abi.I64, rng.integers(-99, 99, 700))])
    dups = _table(rng, 2000, 1000, 0.0)
    cfg = H.join_cfg(T2, T2, [0], [0], abi.JOIN_LEFT_OUTER, 1)
    for build in (uniq, dups):
        stats = []
        got = G.run_join(ctx, cfg, build, probe, chunk_rows=1 << 22, pull_rows=4096, radix=FORCE, packing=FORCE, stats_out=stats)
        assert stats[0].probe_route == abi.ROUTE_PACKED and got.NumRows() == orc.hash_join(cfg, build, probe).NumRows()


def join_keyrec_conds(ctx, orc):
    n = 4000
    rng = np.random.default_rng(4)
    kb = Chunk([Column(abi.I64, rng.integers(0, 600, n)), _words(n, 50, 13), Column(abi.I64, rng.integers(-99, 99, n))])
    kp = Chunk([Column(abi.I64, rng.integers(0, 600, n)), _words(n, 60, 11), Column(abi.I64, rng.integers(-99, 99, n))])
    keep = []
    conds = [E.ScalarFunction("gt", E.ScalarFunction("plus", E.Column(2, abi.I64), E.Column(5, abi.I64)), E.Constant(0))]
    cfg = H.join_cfg(kp.types(), kb.types(), [0, 1], [0, 1], abi.JOIN_LEFT_OUTER, 1, conds, (), keep)
    stats = []
    got = G.run_join(ctx, cfg, kb, kp, chunk_rows=1 << 20, radix=FORCE, stats_out=stats)
    assert stats[0].probe_route == abi.ROUTE_KEYREC and got.NumRows() == orc.hash_join(cfg, kb, kp).NumRows()


def join_varlen(ctx, orc):
    n = 3000
    rng = np.random.default_rng(5)
    build = Chunk([Column(abi.I64, rng.integers(0, 500, n)), _words(n, 977, 7)])
    probe = Chunk([Column(abi.I64, rng.integers(0, 600, n), rng.random(n) > 0.05), _words(n, 31, 5)])
    cfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1)
    assert G.run_join(ctx, cfg, build, probe, chunk_rows=4096).NumRows() == orc.hash_join(cfg, build, probe).NumRows()


def _abandoned_join(ctx, overlap, cancel):
    """host pushes in batches of 4096 rows; the handle is destroyed with result batches still queued (their copies possibly in flight)"""
    rng = np.random.default_rng(6)
    build, probe = _table(rng, 3000, 800), _table(rng, 20_000, 900)
    cfg = H.join_cfg(T2, T2, [0], [0], abi.JOIN_LEFT_OUTER, 1, probe_batch_rows=4096)
    lib = ctx.lib
    ctx.set_knob(abi.KNOB_HOST_OVERLAP, overlap)
    h = C.c_void_p()
    _lib.check(lib.tsq_join_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
    try:
        G.push_chunked(lib.tsq_join_build_push, h, build, 1024)
        _lib.check(lib.tsq_join_build_finish(h), h)
        for lo in range(0, probe.NumRows(), 1024):
            keep = []
            part = probe.slice(lo, lo + 1024)
            _lib.check(lib.tsq_join_probe_push(h, make_cols(part.columns, keep), 2, part.NumRows(), None), h)
        if cancel:
            _lib.check(lib.tsq_join_cancel(h), h)
            n, eos = C.c_int64(0), C.c_int32(0)
            keep = []
            out, _ = out_buffers(T2 + T2, 1024, keep)
            assert lib.tsq_join_pull(h, out, 4, 1024, C.byref(n), C.byref(eos)) == abi.ERR_CANCELLED
    finally:
        lib.tsq_join_destroy(h)
        ctx.set_knob(abi.KNOB_HOST_OVERLAP)


def join_host_push_overlap_abandoned(ctx, orc):
    _abandoned_join(ctx, 1, False)


def join_host_push_one_stream_abandoned(ctx, orc):
    _abandoned_join(ctx, 0, False)


def join_cancelled_before_pull(ctx, orc):
    _abandoned_join(ctx, 1, True)


# ---------------------------------------------------------------- aggregates
AGGS = [(abi.AGG_FIRSTROW, 0, abi.I64), (abi.AGG_SUM, 1, abi.I64), (abi.AGG_COUNT, -1, abi.I64)]


def agg_fast_path(ctx, orc):
    chk = _table(np.random.default_rng(7), 5000, 300)
    cfg = H.agg_cfg(T2, [0], AGGS)
    got = G.run_agg(ctx, cfg, chk, [abi.I64] * 3, chunk_rows=4096, fast=abi.AGGFAST_FORCE)
    assert got.NumRows() == orc.hash_agg(cfg, chk, 4, 4).NumRows()
    ordered = orc.sort_rows(chk, [0], [False])
    assert G.run_agg(ctx, cfg, ordered, [abi.I64] * 3, stream=True).NumRows() == got.NumRows()


def agg_wide_keys(ctx, orc):
    """several integer key columns composed into one 64-bit key handed to a child aggregate (the size its own test engages it at)"""
    from . import test_agg_packed_gpu as P
    spec = P.WIDE_SPECS["q3_like"]
    rng = np.random.default_rng(8)
    chk, types, nk = P._mk_chunk(rng, 150_001, spec)
    for k in range(nk):
        c = chk.columns[k]
        vals = rng.integers(spec[k][1], spec[k][2], 40)
        vals[0], vals[1] = spec[k][1], spec[k][2] - 1
        chk.columns[k] = Column(c.tp, vals[rng.integers(0, 40, len(c))], c.notnull)
    st = P._mk_check(ctx, orc, chk, types, nk, P._mk_aggs(nk, types, "sum_count"), want_packed=None)
    assert st.build_partitioned == 2


def agg_group_id_front(ctx, orc):
    """more than four key columns: a group-id dictionary in front of an inner aggregate, host and device pushes"""
    from . import test_agg_manykeys_gpu as M
    chunk, _ = M.make_input(5000, 7, "nulls5", "sqrt")
    types = chunk.types()
    descs, _ = M.plan_a(7, types)
    want = M.oracle_by_rid(orc, chunk, descs).NumRows()
    assert M.run_host(ctx, chunk, list(range(7)), descs).NumRows() == want
    assert M.run_device(ctx, chunk, list(range(7)), descs).NumRows() == want


def agg_string_keys(ctx, orc):
    n = 4000
    rng = np.random.default_rng(9)
    kb = Chunk([Column(abi.I64, rng.integers(0, 600, n)), _words(n, 50, 13), Column(abi.I64, rng.integers(-99, 99, n))])
    aggs = [(abi.AGG_FIRSTROW, 1, abi.BYTES), (abi.AGG_SUM, 2, abi.I64), (abi.AGG_COUNT, -1, abi.I64)]
    cfg = H.agg_cfg(kb.types(), [1], aggs)
    stats = []
    got = G.run_agg(ctx, cfg, kb, [abi.BYTES, abi.I64, abi.I64], chunk_rows=1 << 20, fast=abi.AGGFAST_FORCE, stats_out=stats)
    assert stats[0].build_partitioned == 3 and got.NumRows() == orc.hash_agg(cfg, kb, 4, 4).NumRows()


# ---------------------------------------------------------------- the other operators
def sort_with_strings(ctx, orc):
    n = 3000
    rng = np.random.default_rng(10)
    chk = Chunk([Column(abi.I64, rng.integers(0, 50, n), rng.random(n) > 0.05), _words(n, 97, 9)])
    assert G.run_sort(ctx, chk, [0, 1], [False, True]).rows() == orc.sort_rows(chk, [0, 1], [False, True]).rows()
    assert G.run_sort(ctx, chk, [1], [False], offset=5, count=100).NumRows() == 100


def expr_and_filter(ctx, orc):
    n = 3000
    rng = np.random.default_rng(11)
    chk = Chunk([_words(n, 40, 7), Column(abi.I64, rng.integers(-99, 99, n))])
    e = E.ScalarFunction("and", E.ScalarFunction("le", E.ScalarFunction("ifnull", E.Column(0, abi.BYTES), E.Constant("w20")), E.Constant("w20w20")),
                         E.ScalarFunction("gt", E.ScalarFunction("plus", E.ScalarFunction("length", E.Column(0, abi.BYTES)), E.Column(1, abi.I64)), E.Constant(0)))
    ce = E.CompiledExpr(ctx, [e])
    try:
        assert ce.VecEval(chk).values() == orc.expr_eval(E.compile_expr(e), chk)[0].values()
        ce.VectorizedFilter(chk)
    finally:
        ce.close()


def project_with_filter(ctx, orc):
    from . import test_select_project_gpu as S
    chk, want = S.main_case(4096)
    S.check(ctx, chk, S.FILTERS, S.OUTPUTS, abi.JIT_OFF, want)


def group_id_dictionary(ctx, orc):
    from . import test_groupid_gpu as T
    n = 3000
    rng = np.random.default_rng(12)
    cols = [Column(abi.I64, rng.integers(0, 40, n), rng.random(n) > 0.05), _words(n, 13, 6), Column(abi.I64, rng.integers(0, 3, n))]
    g = T.GroupId(ctx, [c.tp for c in cols])
    try:
        ids = g.assign(cols)
        count, _ = g.keys()
        assert count == g.count() == int(ids.max()) + 1
    finally:
        g.close()


def analyze_collector_and_histogram(ctx, orc):
    from tinysql_amd.statistics import AnalyzeCollector, SortedBuilder
    n = 3000
    rng = np.random.default_rng(13)
    chk = Chunk([Column(abi.I64, rng.integers(0, 500, n), rng.random(n) > 0.05), _words(n, 97, 9)])
    with AnalyzeCollector(ctx, chk.types(), 100, 1000, 4, 256) as a:
        a.push(chk.slice(0, 1000))
        a.push(chk.slice(1000, n))
        assert len(a.finish()) == 2
    for col in (Column(abi.I64, np.sort(rng.integers(0, 500, n))), StrColumn(sorted(b"s%05d" % v for v in rng.integers(0, 500, n).tolist()))):
        b = SortedBuilder(ctx, col.tp, 16)
        try:
            b.push(col)
            assert b.Hist().TotalRowCount() == n
        finally:
            b.close()


def union_scan(ctx, orc):
    from tinysql_amd import executor as X
    from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceTableScan, GpuUnionScanExec, drain_device
    uh = np.arange(2000, dtype=np.int64) * 2
    ua = uh[::5] + 1
    dirty = X.DirtyTable()
    for h_ in ua:
        dirty.AddRow(h_)
    for h_ in uh[::7]:
        dirty.DeleteRow(h_)
    table = DeviceChunk.from_host(ctx, Chunk([Column(abi.I64, uh), Column(abi.I64, uh * 3)]))
    try:
        us = GpuUnionScanExec(ctx, DeviceTableScan(ctx, table, 512), dirty, Chunk([Column(abi.I64, ua), Column(abi.I64, ua * 3)]), [], 0, False)
        rows = [r for ch in drain_device(us) for r in ch.rows()]
    finally:
        table.free()
    assert len(rows) == len(np.setdiff1d(uh, uh[::7])) + len(ua)


def index_lookup(ctx, orc):
    from tinysql_amd import coprocessor, tablecodec
    from tinysql_amd import rowcodec as RC
    from tinysql_amd.gpu_pipeline import GpuIndexLookUpExecutor, drain_device
    rng = np.random.default_rng(14)
    lh = np.sort(rng.choice(np.arange(-9000, 9000), 3000, replace=False)).astype(np.int64)
    lv, lw = rng.integers(0, 500, 3000), rng.integers(-99, 99, 3000)
    lvals, loffs = tablecodec.EncodeRow(ctx, Chunk([Column(abi.I64, lv), Column(abi.I64, lw)]), [1, 2])
    ltable = coprocessor.DeviceTable(ctx, tablecodec.EncodeRowKeysWithHandles(ctx, 41, lh), lvals, loffs)
    try:
        io = np.lexsort((lh, lv))
        ik, iko, ivl, ivo, _ = tablecodec.GenIndexKeys(ctx, 41, 5, False, Chunk([Column(abi.I64, lv[io])]), lh[io])
        linfo = [RC.ColInfo(1, RC.TypeLonglong), RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(-1, RC.TypeLonglong, IsPKHandle=True)]
        for keep_order in (True, False):
            scan = coprocessor.indexScanExec(ctx, [abi.I64, abi.I64], 1, coprocessor.indexScanExec.PrimaryKeyIsSigned, ik, iko, ivl, ivo)
            lk = GpuIndexLookUpExecutor(ctx, scan, ltable, linfo, [], keep_order, 64, 1024)
            assert sum(ch.NumRows() for ch in drain_device(lk)) == 3000
    finally:
        ltable.close()


def insert_replace_select(ctx, orc):
    """the casts and auto ids of INSERT .. SELECT, then a REPLACE and an INSERT statement through the duplicate-key checker"""
    from tests import cast_ref as CR
    from tests import dupcheck_gpu_helpers as DG
    from tests import dupcheck_ref as DR
    from tinysql_amd import table as TB
    from tinysql_amd.gpu_pipeline import DeviceChunk as DC
    rng = np.random.default_rng(15)
    fts = [CR.FieldType(abi.TP_LONGLONG, not_null=True, auto_increment=True), CR.FieldType(abi.TP_LONG), CR.FieldType(abi.TP_TINY, unsigned=True, not_null=True),
           CR.FieldType(abi.TP_DOUBLE, 8, 2)]
    infos = [TB.ColumnInfo(f.tp, f.flen, f.decimal, (TB.UnsignedFlag if f.unsigned else 0) | (TB.NotNullFlag if f.not_null else 0) |
                           (TB.AutoIncrementFlag if f.auto_increment else 0)) for f in fts]
    m = 3000
    src = Chunk([Column(abi.I64, rng.integers(-(1 << 32), 1 << 32, m), rng.random(m) > 0.1), Column(abi.I64, rng.integers(-5, 300, m)),
                 Column(abi.F64, np.round(rng.uniform(-2e6, 2e6, m), 3), rng.random(m) > 0.1)])
    stmt = TB.StatementContext(TruncateAsWarning=True)
    dsrc = DC.from_host(ctx, src)
    try:
        dcast, _ = TB.CastValue(ctx, dsrc, infos, stmt, [-1, 0, 1, 2])
        try:
            TB.FillAutoID(ctx, dcast.columns[0], m, 10, infos[0], stmt)
        finally:
            dcast.free()
    finally:
        dsrc.free()
    shape = DR.TableShape([abi.I64, abi.I64, abi.BYTES, abi.F64], 0, [[(1, None)], [(2, None)]])
    store = DR.Store(shape)
    DR.replace_stmt(shape, store, [(int(k), int(k) % 400, b"s%d" % (k % 450), 0.5) for k in rng.integers(0, 2000, 500)], 0)
    stored = sorted(store.table().items())
    rows = [(int(k), int(a), b"s%d" % int(w), 0.5) for k, a, w in zip(rng.integers(0, 20000, 3000), rng.integers(0, 30000, 3000), rng.integers(0, 30000, 3000))]
    rows[100:110] = [r for _, r in stored[:10]]
    DG.check_replace(ctx, shape, stored, rows)
    assert DG.check_insert(ctx, shape, stored, rows) is not None


def mvcc_store_and_scans(ctx, orc):
    from tests import mvcc_gpu_helpers as MG
    from tests import mvcc_ref as MR
    store = MR.random_store(np.random.default_rng(9), 500)
    mh = MG.open_store(ctx, store)
    try:
        for ts in (1000, MR.U64_MAX):
            for desc in (False, True):
                MG.check(mh, store, [(b"", b"")], ts, desc)
    finally:
        mh.close()


def mvcc_create_refuses_unordered_keys(ctx, orc):
    from tests import mvcc_ref as MR
    from tinysql_amd import mvcc as M
    with pytest.raises(_lib.TsqError) as e:
        M.MvccStore(ctx, MR.flat_arrays([b"B", b"A"], [5, 5], [0, 0], [0, 0], [b"x", b"y"], [], [], [], [], []))
    assert e.value.status == abi.ERR_INVALID and e.value.message == "mvcc store: keys not ascending"


# ---------------------------------------------------------------- stateless entry points
def row_keys(ctx, orc):
    from tinysql_amd import tablecodec
    hs = np.random.default_rng(16).integers(-(1 << 62), 1 << 62, 3000)
    keys = tablecodec.EncodeRowKeysWithHandles(ctx, 41, hs)
    assert (tablecodec.DecodeRowKeys(ctx, keys) == hs).all()


def row_keys_decode_refuses_an_invalid_key(ctx, orc):
    from tinysql_amd import tablecodec
    keys = np.array(tablecodec.EncodeRowKeysWithHandles(ctx, 41, np.arange(3000, dtype=np.int64)), dtype=np.uint8, copy=True)
    keys[19 * 1500] ^= 0xFF  # the table prefix of key 1500
    with pytest.raises(_lib.TsqError) as e:
        tablecodec.DecodeRowKeys(ctx, keys)
    assert e.value.status == abi.ERR_INVALID


def stored_rows(ctx, orc):
    """rowcodec: the decoder of a table scan, the encoder of the write path and the index entries"""
    from tinysql_amd import rowcodec as RC
    from tinysql_amd import tablecodec
    n = 3000
    rng = np.random.default_rng(17)
    chk = Chunk([Column(abi.I64, rng.integers(0, 3000, n), rng.random(n) > 0.05), _words(n, 40, 7), Column(abi.I64, rng.integers(-99, 99, n))])
    vals, offs = tablecodec.EncodeRow(ctx, chk, [1, 2, 300])
    ovals, ooffs = orc.rowcodec_encode(chk, [1, 2, 300])
    assert bytes(vals) == bytes(ovals) and (offs == ooffs).all()
    infos = [RC.ColInfo(300, RC.TypeLonglong), RC.ColInfo(2, RC.TypeVarchar), RC.ColInfo(1, RC.TypeLonglong)]
    assert RC.NewChunkDecoder(ctx, infos).DecodeToChunk(vals, offs).NumRows() == n
    tablecodec.GenIndexKeys(ctx, 41, 3, True, Chunk(chk.columns[:2]), np.arange(n, dtype=np.int64) - 7)


def responses_and_wire_chunks(ctx, orc):
    from tinysql_amd import chunk_codec, distsql
    n = 3000
    rng = np.random.default_rng(18)
    chk = Chunk([Column(abi.I64, rng.integers(0, 3000, n), rng.random(n) > 0.05), _words(n, 40, 7), Column(abi.I64, rng.integers(-99, 99, n))])
    raw, offs = distsql.encode_rows(ctx, chk)
    assert bytes(raw) == bytes(orc.encode_rows(chk))
    assert distsql.decode_chunks(ctx, distsql.response_chunks(raw, offs), chk.types()).rows() == chk.rows()
    fixed = Chunk([chk.columns[0], chk.columns[2]])
    fraw = orc.encode_rows(fixed)
    dec, used = distsql.decode_rows(ctx, fraw, fixed.types(), n)
    assert used == fraw.size and dec.NumRows() == n
    wire = chunk_codec.Codec(ctx, chk.types()).Encode(chk)
    assert wire == orc.WireChunk.from_chunk(chk).encode()
    assert chunk_codec.Codec(ctx, chk.types()).Decode(wire)[0].to_chunk().rows() == chk.rows()


KINDS = [join_table_route, join_radix_route, join_packed_count, join_packed_rows, join_keyrec_conds, join_varlen, join_host_push_overlap_abandoned,
         join_host_push_one_stream_abandoned, join_cancelled_before_pull, agg_fast_path, agg_wide_keys, agg_group_id_front, agg_string_keys,
         sort_with_strings, expr_and_filter, project_with_filter, group_id_dictionary, analyze_collector_and_histogram, union_scan, index_lookup,
         insert_replace_select, mvcc_store_and_scans, mvcc_create_refuses_unordered_keys, row_keys, row_keys_decode_refuses_an_invalid_key, stored_rows,
         responses_and_wire_chunks]


@pytest.mark.parametrize("kind", KINDS, ids=lambda k: k.__name__)
def test_nothing_stays_in_the_arena(actx, orc, kind):
    actx.reserve(0)  # (refused while a buffer of an earlier kind is still alive)
    actx.reserve(ARENA)
    assert actx.arena_stats() == {"size": ARENA, "used": 0, "peak": 0}
    kind(actx, orc)
    st = actx.arena_stats()
    assert st["used"] == 0, "%s left %d bytes of the arena in use" % (kind.__name__, st["used"])
    assert st["peak"] > 0, "%s never took a buffer from the arena" % kind.__name__
