"""GPU: a statement's row stream goes from GpuInsertSelectExec into the store without leaving HBM — INSERT .. SELECT over a PK-handle
table without secondary indexes, mvcc.write_insert_batches (prewrite + commit of the batches' record keys and stored rows as
device-resident requests), then tableScanExec.from_store on the next store: at commitTS the inserted rows together with the old
ones, at commitTS - 1 only the old ones.  A second statement whose handles meet a foreign lock raises ErrLocked and leaves the store
as it was.  The model (tests/mvcc_ref.py) is fed the same pairs from the batches' host copies."""
import numpy as np
import pytest

from tests import mvcc_gpu_helpers as G
from tests import mvcc_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import mvcc_write_ref as W
from tinysql_amd import _abi as abi
from tinysql_amd import coprocessor as cop
from tinysql_amd import mvcc as M
from tinysql_amd import rowcodec as RC
from tinysql_amd import table as T
from tinysql_amd import tablecodec
from tinysql_amd.chunk import Chunk, Column
from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceTableScan, GpuInsertSelectExec, InsertTableInfo, drain_device

pytestmark = pytest.mark.gpu

TID = 41
SCAN_COLS = [RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(3, RC.TypeDouble), RC.ColInfo(1, RC.TypeLonglong, 0, True)]
N_OLD = 3000


def table_info():
    cols = [T.ColumnInfo(abi.TP_LONGLONG, Flag=T.NotNullFlag | T.PriKeyFlag), T.ColumnInfo(abi.TP_LONGLONG), T.ColumnInfo(abi.TP_DOUBLE)]
    return InsertTableInfo(TID, cols, [1, 2, 3], PKIsHandle=True, pk_offset=0)


def old_store(ctx):
    """handles 0, 2, 4, ..: rows committed at 10, every 9th rewritten at 15"""
    handles = np.arange(N_OLD, dtype=np.int64) * 2
    keys = [bytes(r) for r in np.asarray(tablecodec.EncodeRowKeysWithHandles(ctx, TID, handles)).reshape(-1, 19)]
    a, b = handles * 10, handles / 4.0
    vals, offs = tablecodec.EncodeRow(ctx, Chunk([Column(abi.I64, a), Column(abi.F64, b)]), [2, 3])
    raw = bytes(vals)
    s = R.Store()
    for i, k in enumerate(keys):
        v = raw[offs[i]:offs[i + 1]]
        s.versions[k] = ([R.Value(R.PUT, 14, 15, v)] if i % 9 == 0 else []) + [R.Value(R.PUT, 9, 10, v)]
    return s, {int(h): (int(x), float(y)) for h, x, y in zip(handles, a, b)}


def statement(ctx, handles, batch_rows):
    """the InsertBatches of INSERT INTO t (id, a, b) SELECT .. with the given ascending handles -> (batches, {handle: (a, b)})"""
    a, b = handles * 7 + 1, handles / 8.0
    dt = DeviceChunk.from_host(ctx, Chunk([Column(abi.I64, handles), Column(abi.I64, a), Column(abi.F64, b)]))
    ex = GpuInsertSelectExec(ctx, DeviceTableScan(ctx, dt, batch_rows), table_info(), [0, 1, 2], [], T.StatementContext())
    batches = []
    try:
        ex.Open()
        while True:
            bt = ex.Next()
            if bt is None:
                break
            batches.append(bt)
    finally:
        ex.Close()
        dt.free()
    return batches, {int(h): (int(x), float(y)) for h, x, y in zip(handles, a, b)}


def model_puts(s, batches, primary, start_ts, commit_ts=None):
    for bt in batches:
        keys, (raw, offs), _ = bt.to_host()
        raw = bytes(raw)
        muts = [(R.OP_PUT, bytes(keys[i]), raw[offs[i]:offs[i + 1]]) for i in range(bt.n)]
        assert W.prewrite(s, muts, primary, start_ts)[1]
    if commit_ts is not None:
        for bt in batches:
            keys = bt.to_host()[0]
            assert W.commit(s, [bytes(k) for k in keys], start_ts, commit_ts)[1]


def scan_rows(ctx, ms, ts):
    prefix = tablecodec.EncodeRowKeysWithHandles(ctx, TID, np.zeros(1, dtype=np.int64))
    prefix = bytes(np.asarray(prefix))[:11]
    e = cop.tableScanExec.from_store(ctx, SCAN_COLS, ms, [(prefix + b"\x00", cop.PrefixNext(prefix))], ts)
    rows = {}
    for c in drain_device(e):
        for a, b, h in c.rows():
            rows[h] = (a, b)
    return rows, e.Counts()


def test_insert_select_becomes_visible_to_the_snapshot_read_without_a_host_round_trip(ctx):
    s, old_rows = old_store(ctx)
    ms = WG.open_rw(ctx, s)
    # new handles interleaved with the store's, some equal to existing ones (rewritten), some behind the last key; three batches
    handles = np.unique(np.concatenate([np.arange(1, 4000, 2), np.arange(0, 600, 6), np.arange(2 * N_OLD, 2 * N_OLD + 500)])).astype(np.int64)
    batches, new_rows = statement(ctx, handles, 1024)
    nxt = None
    try:
        assert len(batches) >= 3
        primary = bytes(batches[0].to_host()[0][0])
        nxt = M.write_insert_batches(ms, batches, primary, 20, 25, ttl=5)
        model_puts(s, batches, primary, 20, 25)
        WG.compare_store(nxt, s)
        got, counts = scan_rows(ctx, nxt, 25)
        want = dict(old_rows)
        want.update(new_rows)
        assert got == want and counts == [len(want)] and len(want) == N_OLD + len(handles) - 100
        got, counts = scan_rows(ctx, nxt, 24)
        assert got == old_rows and counts == [N_OLD]
        got, _ = scan_rows(ctx, ms, 25)  # the store the statement was written from is as it was
        assert got == old_rows
        G.check(nxt, s, [(b"", b"")], 25)
    finally:
        for bt in batches:
            bt.free()
        if nxt is not None:
            nxt.close()
        ms.close()


def test_a_statement_that_meets_a_foreign_lock_raises_and_leaves_the_store(ctx):
    s, old_rows = old_store(ctx)
    locked = bytes(np.asarray(tablecodec.EncodeRowKeysWithHandles(ctx, TID, np.array([2501], dtype=np.int64))))
    s.locks[locked] = R.Lock(30, b"their-primary", b"theirs", R.OP_PUT, 77)
    ms = WG.open_rw(ctx, s)
    handles = np.arange(1, 4000, 2, dtype=np.int64)  # 2501 is row 226 of the second batch: one prewrite succeeds before it
    batches, _ = statement(ctx, handles, 1024)
    try:
        with pytest.raises(M.ErrLocked) as e:
            M.write_insert_batches(ms, batches, b"mine", 40, 45)
        assert (e.value.RawKey, e.value.Primary, e.value.StartTS, e.value.TTL, e.value.LockType) == (locked, b"their-primary", 30, 77, R.OP_PUT)
        assert e.value.Key == R.mvcc_encode(locked, R.LOCK_VER)
        at = int(np.flatnonzero(handles[1024:2048] == 2501)[0])
        assert e.value.errors[at] is e.value and sum(x is not None for x in e.value.errors) == 1
        WG.compare_store(ms, s)
        got, _ = scan_rows(ctx, ms, 29)
        assert got == old_rows
        # a conflict: the same statement below the store's newest commitTS (15 on every 9th row; handle 0 is one)
        with pytest.raises(M.ErrConflict) as e:
            b2, _ = statement(ctx, np.arange(0, 40, 2, dtype=np.int64), 1024)
            try:
                M.write_insert_batches(ms, b2, b"mine", 12, 13)
            finally:
                for bt in b2:
                    bt.free()
        assert (e.value.StartTS, e.value.ConflictTS, e.value.ConflictCommitTS) == (12, 14, 15)
        WG.compare_store(ms, s)
    finally:
        for bt in batches:
            bt.free()
        ms.close()
