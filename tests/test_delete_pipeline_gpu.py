"""GPU: DELETE .. WHERE goes from a scan of the store to a committed next store without a key byte crossing to the host:
tableScanExec.from_store -> selectionExec -> GpuDeleteExec pushes, per chunk, the record keys and the keys of both indexes as DELETE
entries into the transaction buffer (kv.MemBuffer); mvcc.write_membuffer prewrites and commits them.  Table t (id PK handle, a BIGINT,
s VARCHAR NULL), a non-unique index on a, a unique index on s (a NULL s takes the handle-suffixed key); about 3000 rows.

The statement is DELETE FROM t WHERE a % 3 = 0.  The expression evaluator has no MOD signature; over a's domain here, [0, 50), the
predicate is written as IN lists of the multiples of 3, which select exactly the rows a % 3 = 0 selects."""
import numpy as np
import pytest

from tests import membuf_ref as MR
from tests import mvcc_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import mvcc_write_ref as W
from tests import txn_pipeline_helpers as P
from tinysql_amd import _abi as abi
from tinysql_amd import coprocessor as cop
from tinysql_amd import expression as E
from tinysql_amd import kv
from tinysql_amd import mvcc as M
from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceTableScan, GpuDeleteExec

pytestmark = pytest.mark.gpu

IN = lambda vals: E.ScalarFunction("in", E.Column(1, abi.I64), *[E.Constant(v) for v in vals])
WHERE = [E.ScalarFunction("or", IN(range(0, 27, 3)), IN(range(27, 50, 3)))]  # (two lists: one of 17 items is deeper than the evaluator's stack)


def delete_where(ctx, ms, mb, ts, batch_rows=1024):
    scan = cop.tableScanExec.from_store(ctx, P.SCAN_COLS, ms, [(P.RECORD_PREFIX + b"\x00", cop.PrefixNext(P.RECORD_PREFIX))], ts, batch_rows=batch_rows)
    ex = GpuDeleteExec(ctx, cop.selectionExec(ctx, scan, WHERE), P.table_info(), P.INDICES, 0, mb)
    ex.Open()
    try:
        while ex.Next().NumRows():
            raise AssertionError("a DELETE returns no rows")
    finally:
        ex.Close()
    return ex.affectedRows


def model_deletes(model, orc, rows):
    for stream in P.kv_pairs(orc, rows):
        for k, _ in stream:
            model.Delete(k)


def stored(ctx, orc):
    rows = P.make_rows(np.random.default_rng(67).choice(np.arange(-5000, 5000), 3000, replace=False))
    return rows, P.committed_store(orc, rows, 9, 10)


def test_delete_where_commits_from_hbm(ctx, orc):
    rows, s = stored(ctx, orc)
    gone = {h: r for h, r in rows.items() if r[0] % 3 == 0}
    assert 900 < len(gone) < 1200 and any(r[1] is None for r in gone.values())
    ms = WG.open_rw(ctx, s)
    nxt = None
    with kv.MemBuffer(ctx) as mb:
        try:
            assert delete_where(ctx, ms, mb, 30) == len(gone)
            model = MR.Model()
            model_deletes(model, orc, gone)
            want = model.finish()
            got = mb.finish()
            assert (got["n_entries"], got["puts"], got["dels"], got["locks"]) == (3 * len(gone), 0, 3 * len(gone), 0) and mb.entries() == want["entries"]
            nxt = M.write_membuffer(ms, mb, 30, 35)
            assert W.prewrite(s, want["entries"], want["primary"], 30)[1] and W.commit(s, [e[1] for e in want["entries"]], 30, 35)[1]
            WG.compare_store(nxt, s)
            left = {h: r for h, r in rows.items() if h not in gone}
            assert P.read_back(ctx, nxt, 35) == P.expect_read(left)   # the rows and all their index entries are gone
            assert P.read_back(ctx, nxt, 34) == P.expect_read(rows)   # ... and all there one tick earlier
        finally:
            if nxt is not None:
                nxt.close()
            ms.close()


def test_insert_then_delete_in_one_transaction_gives_op_del(ctx, orc):
    """rows inserted into the buffer and deleted again by the same transaction: Set then Delete on the record key and on both index keys
    leaves Op_Del, not a put"""
    handles = np.arange(100, 700, dtype=np.int64)
    rows = P.make_rows(handles)
    gone = {h: r for h, r in rows.items() if r[0] % 3 == 0}
    with kv.MemBuffer(ctx) as mb:
        P.insert_into(ctx, mb, rows, handles[::-1].copy(), batch_rows=256)
        chunk, _ = P.rows_chunk(rows)
        dt = DeviceChunk.from_host(ctx, chunk)
        ex = GpuDeleteExec(ctx, cop.selectionExec(ctx, DeviceTableScan(ctx, dt, 256), WHERE), P.table_info(), P.INDICES, 0, mb)
        try:
            ex.Open()
            while ex.Next().NumRows():
                pass
        finally:
            ex.Close()
            dt.free()
        assert ex.affectedRows == len(gone)
        model = MR.Model()
        P.model_sets(model, orc, rows)
        model_deletes(model, orc, gone)
        want = model.finish()
        got = mb.finish()
        assert mb.entries() == want["entries"] and (got["puts"], got["dels"]) == (3 * (len(rows) - len(gone)), 3 * len(gone))
        ops = {k: op for op, k, _ in mb.entries()}
        for stream in P.kv_pairs(orc, gone):
            assert all(ops[k] == abi.MVCC_OP_DEL for k, _ in stream)
        ms = WG.open_rw(ctx, R.Store())
        try:
            nxt = M.write_membuffer(ms, mb, 3, 4)
            try:
                assert P.read_back(ctx, nxt, 4) == P.expect_read({h: r for h, r in rows.items() if h not in gone})
            finally:
                nxt.close()
        finally:
            ms.close()


def test_foreign_lock_on_an_index_key_raises_errlocked_and_leaves_the_store(ctx, orc):
    rows, s = stored(ctx, orc)
    victim = sorted(h for h, r in rows.items() if r[0] % 3 == 0)[17]
    locked = P.kv_pairs(orc, {victim: rows[victim]})[1][0][0]  # the row's key in the index on a
    s.locks[locked] = R.Lock(31, b"their-primary", b"0", R.OP_PUT, 77)
    ms = WG.open_rw(ctx, s)
    with kv.MemBuffer(ctx) as mb:
        try:
            delete_where(ctx, ms, mb, 30)  # (the read at 30 is below the lock's startTS: it does not meet it)
            with pytest.raises(M.ErrLocked) as e:
                M.write_membuffer(ms, mb, 40, 45)
            assert (e.value.RawKey, e.value.Primary, e.value.StartTS, e.value.TTL, e.value.LockType) == (locked, b"their-primary", 31, 77, R.OP_PUT)
            assert sum(x is not None for x in e.value.errors) == 1
            WG.compare_store(ms, s)
            assert P.read_back(ctx, ms, 30) == P.expect_read(rows)
        finally:
            ms.close()
