"""GPU: read your own writes without the host.  The three mem readers (gpu_pipeline.memTableReader / memIndexReader /
memIndexLookUpReader) over a finished kv.MemBuffer and GpuUnionScanExec.from_membuffer (tsq_membuf_dirty -> tsq_unionscan_create_dev,
the reader's chunk -> tsq_unionscan_set_added):
  * the steps of executor/union_scan_test.go (tests/golden/memread_cases.json), expecting the fixture's rows;
  * end to end: 2^14 committed rows in an MVCC store, table t (id PK handle, a BIGINT, s VARCHAR NULL; a BIGINT index, a unique
    8-byte-string index), 1000 rows inserted through InsertBatch.write_to(membuf), 1000 rows deleted by GpuDeleteExec (50 of them
    inserted a moment ago); every reader, ascending and descending, with and without a condition, signed and unsigned PK handle,
    equals (1) tests/memread_ref.py + UnionScanRef and (2) the same reader WITHOUT a union scan over the store the buffer commits to,
    read at commitTS — "union scan over snapshot + buffer = plain scan after commit", which needs no model."""
import functools

import numpy as np
import pytest

from tests import membuf_ref as MR
from tests import memread_cases as K
from tests import memread_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import test_unionscan_gpu as UG
from tests import txn_pipeline_helpers as T
from tests.unionscan_ref import UnionScanRef
from tinysql_amd import _abi as abi
from tinysql_amd import coprocessor as cop
from tinysql_amd import expression as E
from tinysql_amd import gpu_pipeline as P
from tinysql_amd import kv
from tinysql_amd import mvcc as M
from tinysql_amd import rowcodec as RC

pytestmark = pytest.mark.gpu


def rows_of(exe):
    return [r for c in P.drain_device(exe) for r in c.rows()]


def chunk_rows(chunk):
    try:
        return chunk.to_host().rows() if chunk.NumRows() else []
    finally:
        chunk.free()


# ------------------------------------------------------------------------------------------------ the reference's own rows
def fixture_reader(ctx, mb, layout, rd, conditions=None):
    if rd.kind == "table":
        return lambda: P.memTableReader(ctx, mb, layout.col_infos(), rd.ranges, rd.desc, conditions)
    if rd.kind == "index":
        return lambda: P.memIndexReader(ctx, mb, rd.types, layout.pk_status, list(range(len(rd.types))), rd.ranges, rd.desc, conditions)
    return lambda: P.memIndexLookUpReader(ctx, mb, layout.index_types(rd.index), layout.pk_status, layout.id, layout.col_infos(), rd.ranges, rd.desc, conditions)


@pytest.mark.parametrize("case", K.golden(), ids=[c["name"] for c in K.golden()])
def test_fixture_steps_through_the_gpu_mem_readers(ctx, orc, case):
    layout, model = K.Layout(case["table"]), MR.Model()
    with kv.MemBuffer(ctx) as mb:
        txn = K.Txn(orc, layout, case["committed"], [model, mb])
        for step in case["steps"]:
            if "insert" in step:
                txn.insert(step["insert"])
            elif "delete" in step:
                txn.delete(step["delete"])
            else:
                rd = K.Read(layout, txn, step["read"])
                # the reader alone, the conditions applied by the reader itself: the restatement's rows
                assert chunk_rows(fixture_reader(ctx, mb, layout, rd, rd.conditions)()) == rd.model_rows(orc, layout, model), step
                exe = P.GpuUnionScanExec.from_membuffer(ctx, UG.ListSource(ctx, rd.types, [rd.snapshot]), mb, layout.id, fixture_reader(ctx, mb, layout, rd),
                                                        rd.used_index, rd.handle_idx, rd.desc, rd.conditions)
                assert rd.project(rows_of(exe)) == rd.expect, step


# ------------------------------------------------------------------------------------------------ end to end
N_STORED, N_NEW, N_DEL, N_DEL_NEW = 1 << 14, 1000, 1000, 50
TS_READ, TS_START, TS_COMMIT = 20, 30, 35
A_MIN = 24  # the condition: a > 24 (about half of the rows; a = handle mod 50)


class World:
    """the store, the buffer after the two statements, the model of both, and the store after the buffer's commit"""

    def __init__(self, ctx, orc):
        self.ctx, self.orc = ctx, orc
        rng = np.random.default_rng(71)
        hs = rng.permutation(40000)  # handles >= 0: the same bytes read through a signed and through an unsigned PK-handle column
        self.rows = T.make_rows(np.sort(hs[:N_STORED]))
        self.new = T.make_rows(hs[N_STORED:N_STORED + N_NEW])
        gone = list(rng.choice(sorted(self.rows), N_DEL - N_DEL_NEW, replace=False)) + list(rng.choice(sorted(self.new), N_DEL_NEW, replace=False))
        everything = {**self.rows, **self.new}
        self.gone = {int(h): everything[int(h)] for h in gone}
        self.ms = WG.open_rw(ctx, T.committed_store(orc, self.rows, 9, 10))
        self.mb = kv.MemBuffer(ctx)
        self.nxt = None
        # INSERT .. SELECT of the new rows, then DELETE of 1000 rows, both into the buffer without a key byte on the host
        T.insert_into(ctx, self.mb, self.new, rng.permutation(sorted(self.new)), batch_rows=256)
        chunk, _ = T.rows_chunk(self.gone)
        dt = P.DeviceChunk.from_host(ctx, chunk)
        ex = P.GpuDeleteExec(ctx, P.DeviceTableScan(ctx, dt, 256), T.table_info(), T.INDICES, 0, self.mb)
        try:
            ex.Open()
            while ex.Next().NumRows():
                pass
        finally:
            ex.Close()
            dt.free()
        assert ex.affectedRows == N_DEL
        self.model = MR.Model()
        T.model_sets(self.model, orc, self.new)
        for stream in T.kv_pairs(orc, self.gone):
            for k, _ in stream:
                self.model.Delete(k)
        assert self.mb.entries() == self.model.finish()["entries"]
        self.dirty = R.dirty_sets(self.model, T.TID)
        assert len(self.dirty[0]) == N_NEW - N_DEL_NEW and len(self.dirty[1]) == N_DEL
        self.sorted_snapshots = {}
        self.tables = {}

    def committed(self):
        """the store after prewrite + commit of the buffer (the buffer stays finished and readable)"""
        if self.nxt is None:
            self.nxt = M.write_membuffer(self.ms, self.mb, TS_START, TS_COMMIT)
        return self.nxt

    def device_table(self, store, ts):
        """the record pairs of `store` at ts as a coprocessor.DeviceTable (the table side of the double read)"""
        if (id(store), ts) not in self.tables:
            p = store.scan([(T.RECORD_PREFIX + b"\x00", cop.PrefixNext(T.RECORD_PREFIX))], ts)
            try:
                pairs = p.to_host()
            finally:
                p.free()
            vals, offs = R._pack([v for _, v in pairs])
            self.tables[(id(store), ts)] = cop.DeviceTable(self.ctx, np.frombuffer(b"".join(k for k, _ in pairs), dtype=np.uint8), vals, offs)
        return self.tables[(id(store), ts)]

    def snapshot(self, which, order):
        """the committed rows in the reader's schema, ascending in its scan order"""
        if which not in self.sorted_snapshots:
            mk = {"table": lambda h, r: (h, r[0], r[1]), "table-by-a": lambda h, r: (h, r[0], r[1]), "a": lambda h, r: (r[0], h), "s": lambda h, r: (r[1], h)}[which]
            self.sorted_snapshots[which] = sorted((mk(h, r) for h, r in self.rows.items()), key=order)
        return self.sorted_snapshots[which]

    def close(self):
        for t in self.tables.values():
            t.close()
        if self.nxt is not None and self.nxt is not self.ms:
            self.nxt.close()
        self.mb.close()
        self.ms.close()


@pytest.fixture(scope="module")
def world(ctx, orc):
    w = World(ctx, orc)
    yield w
    w.close()


def plan(kind, unsigned):
    """per reader: the schema, the order, the ranges, the condition"""
    ht = abi.U64 if unsigned else abi.I64
    cols = [RC.ColInfo(1, RC.TypeLonglong, RC.UnsignedFlag if unsigned else 0, True), RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(3, RC.TypeVarchar)]
    gt = lambda c: [E.ScalarFunction("gt", E.Column(c, abi.I64), E.Constant(A_MIN))]
    d = dict(cols=cols, pk=2 if unsigned else 1)
    if kind == "table":
        d.update(types=[ht, abi.I64, abi.BYTES], used=[], handle=0, snap="table", ranges=[(T.RECORD_PREFIX + b"\x00", cop.PrefixNext(T.RECORD_PREFIX))],
                 cond=gt(1), pred=lambda r: r[1] is not None and r[1] > A_MIN)
    elif kind == "index_a":
        p = T.index_prefix(T.IDX_A)
        d.update(types=[abi.I64, ht], used=[0], handle=1, snap="a", ranges=[(p + b"\x00", cop.PrefixNext(p))], cond=gt(0), pred=lambda r: r[0] > A_MIN, unique=False)
    elif kind == "index_s":
        p = T.index_prefix(T.IDX_S)
        d.update(types=[abi.BYTES, ht], used=[0], handle=1, snap="s", ranges=[(p + b"\x00", cop.PrefixNext(p))], unique=True,
                 cond=[E.ScalarFunction("not", E.ScalarFunction("isnull", E.Column(0, abi.BYTES)))], pred=lambda r: r[0] is not None)
    else:  # the double read through the index on a: the table's schema in the index's order
        p = T.index_prefix(T.IDX_A)
        d.update(types=[ht, abi.I64, abi.BYTES], used=[1], handle=0, snap="table", ranges=[(p + b"\x00", cop.PrefixNext(p))], cond=gt(1),
                 pred=lambda r: r[1] > A_MIN, index_types=[abi.I64, ht], unique=False)
    return d


def store_reader(w, kind, pl, store, ts, desc, cond):
    """the reader over an MVCC store, the conditions where the reference's plan has them"""
    ctx = w.ctx
    if kind == "table":
        e = cop.tableScanExec.from_store(ctx, pl["cols"], store, pl["ranges"], ts, desc, batch_rows=4096)
        return cop.selectionExec(ctx, e, cond) if cond else e
    if kind in ("index_a", "index_s"):
        e = cop.indexScanExec.from_store(ctx, pl["types"], 1, pl["pk"], store, pl["ranges"], ts, desc, batch_rows=4096, unique=pl["unique"])
        return cop.selectionExec(ctx, e, cond) if cond else e
    idx = cop.indexScanExec.from_store(ctx, pl["index_types"], 1, pl["pk"], store, pl["ranges"], ts, desc, batch_rows=4096)
    return P.GpuIndexLookUpExecutor(ctx, idx, w.device_table(store, ts), pl["cols"], cond, True, 1024, 4096)


def mem_reader(w, kind, pl, desc):
    ctx, mb = w.ctx, w.mb
    if kind == "table":
        return lambda: P.memTableReader(ctx, mb, pl["cols"], pl["ranges"], desc)
    if kind in ("index_a", "index_s"):
        return lambda: P.memIndexReader(ctx, mb, pl["types"], pl["pk"], [0, 1], pl["ranges"], desc)
    return lambda: P.memIndexLookUpReader(ctx, mb, pl["index_types"], pl["pk"], T.TID, pl["cols"], pl["ranges"], desc)


def model_added(w, kind, pl, desc, pred):
    specs = [(c.ID, c.tsq_type(), abi.RC_HANDLE if c.IsPKHandle else 0, 0) for c in pl["cols"]]
    if kind == "table":
        return R.mem_table_reader(w.orc, w.model, specs, pl["ranges"], desc, pred)
    if kind in ("index_a", "index_s"):
        return R.mem_index_reader(w.orc, w.model, pl["types"], pl["pk"], [0, 1], pl["ranges"], desc, pred)
    return R.mem_index_lookup_reader(w.orc, w.model, pl["index_types"], pl["pk"], T.TID, specs, pl["ranges"], desc, pred)


@pytest.mark.parametrize("unsigned", [False, True], ids=["signed", "unsigned"])
@pytest.mark.parametrize("with_cond", [False, True], ids=["all", "cond"])
@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("kind", ["table", "index_a", "index_s", "lookup_a"])
def test_read_your_own_writes(world, kind, desc, with_cond, unsigned):
    w, pl = world, plan(kind, unsigned)
    ctx = w.ctx
    cond, pred = (pl["cond"], pl["pred"]) if with_cond else ([], None)
    child = store_reader(w, kind, pl, w.ms, TS_READ, desc, cond)
    exe = P.GpuUnionScanExec.from_membuffer(ctx, child, w.mb, T.TID, mem_reader(w, kind, pl, desc), pl["used"], pl["handle"], desc, cond, pull_rows=1 << 13)
    got = rows_of(exe)
    assert len(got) > 4000 and exe.membuf is not None

    # 1) the restatement: the mem reader's rows and the buffer's dirty handles through UnionScanRef over the committed rows
    asc = functools.cmp_to_key(UnionScanRef(pl["types"], [], [], [], pl["used"], pl["handle"], False).scan_cmp)
    snap = w.snapshot("table-by-a" if kind == "lookup_a" else pl["snap"], asc)
    snap = [r for r in (snap[::-1] if desc else snap) if pred is None or pred(r)]
    ref = UnionScanRef(pl["types"], w.dirty[0], w.dirty[1], model_added(w, kind, pl, desc, pred), pl["used"], pl["handle"], desc)
    want = ref.run([snap])
    assert got == want

    # 2) the invariant: the same reader, no union scan, over the store the buffer commits to, read at commitTS
    assert rows_of(store_reader(w, kind, pl, w.committed(), TS_COMMIT, desc, cond)) == got
