"""GPU: DeviceTableScan -> GpuInsertSelectExec(store=...) — INSERT INTO t SELECT .. into a table with a primary key and unique indexes, the
duplicate-key check of tables.AddRecord included (coprocessor.DeviceTable / DeviceIndex hold the store, dupcheck.DupChecker decides).
The store is what the same executor wrote for an earlier statement; the outcome — every batch, or the statement's ErrKeyExists with its
row, stream and handle — is held to the sequential model of tests/dupcheck_ref.py."""
import numpy as np
import pytest

from tests import dupcheck_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import coprocessor
from tinysql_amd import table as T
from tinysql_amd.dupcheck import KeyExistsError
from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceTableScan, GpuInsertSelectExec, InsertIndexInfo, InsertTableInfo

pytestmark = pytest.mark.gpu

TABLE_ID = 41  # (the model's keys carry tests/dupcheck_ref.py's table id)
INDICES = [InsertIndexInfo(1, True, [1]), InsertIndexInfo(9, False, [1, 2]), InsertIndexInfo(2, True, [2])]  # unique (a), plain (a, s), unique (s)
TYPES = [abi.I64, abi.I64, abi.BYTES]


def table_info(pk):
    cols = [T.ColumnInfo(abi.TP_LONGLONG, Flag=(T.NotNullFlag | T.PriKeyFlag) if pk else 0), T.ColumnInfo(abi.TP_LONGLONG),
            T.ColumnInfo(abi.TP_VARCHAR, 40, Charset="utf8mb4")]
    return InsertTableInfo(TABLE_ID, cols, [1, 2, 3], PKIsHandle=pk, pk_offset=0 if pk else -1)


def shape_of(pk):
    return R.TableShape(TYPES, 0 if pk else None, [[(1, None)], [(2, None)]], TABLE_ID)


def run(ctx, pk, rows, batch_rows, store=None, rowid_base=0, **kw):
    """-> (executor, [(batch rows, record keys, (values, offsets), index KVs)] on the host)"""
    dt = DeviceChunk.from_host(ctx, R.chunk_of(TYPES, rows))
    ex = GpuInsertSelectExec(ctx, DeviceTableScan(ctx, dt, batch_rows), table_info(pk), [0, 1, 2], INDICES, T.StatementContext(), rowid_base=rowid_base, store=store, **kw)
    out = []
    try:
        ex.Open()
        while True:
            b = ex.Next()
            if b is None:
                break
            try:
                hs = np.zeros(b.n, np.int64)
                ctx.d2h(hs, b.handles)
                out.append((b.rows.to_host().rows(), hs) + b.to_host())
            finally:
                b.free()
        return ex, out
    finally:
        ex.Close()
        dt.free()


class Stored:
    """the table an earlier INSERT .. SELECT wrote, uploaded as the storage side holds it: record KV pairs in handle order, each unique
    index's KV pairs in key order"""

    def __init__(self, ctx, pk, rows):
        _, out = run(ctx, pk, rows, 1 << 20)
        (got_rows, hs, keys, (vals, offs), idx), = out
        assert (np.diff(hs) > 0).all()
        self.rows = list(zip(hs.tolist(), got_rows))
        self.rowid_base = 0 if pk else len(rows)
        self.table = coprocessor.DeviceTable(ctx, keys.reshape(-1), vals, offs)
        self.unique = []
        for ix, (ik, iko, iv, ivo, _) in zip(INDICES, idx):
            if not ix.Unique:
                continue
            kb, vb = bytes(ik), bytes(iv)
            ent = sorted((kb[iko[r]:iko[r + 1]], vb[ivo[r]:ivo[r + 1]]) for r in range(len(rows)))
            ko, vo = np.zeros(len(ent) + 1, np.int64), np.zeros(len(ent) + 1, np.int64)
            np.cumsum([len(k) for k, _ in ent], out=ko[1:])
            np.cumsum([len(v) for _, v in ent], out=vo[1:])
            self.unique.append(coprocessor.DeviceIndex(ctx, b"".join(k for k, _ in ent), ko, b"".join(v for _, v in ent), vo))
        self.store = (self.table, self.unique)

    def close(self):
        self.table.close()
        for u in self.unique:
            u.close()


def stored_rows(pk, m=400):
    """m rows; some with a NULL in a unique column (entries that are not distinct)"""
    return [(10 * k if pk else None, None if k % 17 == 0 else 3 * k, None if k % 13 == 0 else b"s%05d" % k) for k in range(m)]


def fresh_rows(n, lo=100000):
    return [(lo + r, lo + r, b"n%07d" % r) for r in range(n)]


@pytest.mark.parametrize("pk", [True, False])
def test_statement_outcomes_equal_the_model(ctx, pk):
    base_rows = stored_rows(pk)
    st = Stored(ctx, pk, base_rows)
    shape = shape_of(pk)
    try:
        assert st.unique[0].n == sum(r[1] is not None for r in base_rows) and st.unique[1].n == sum(r[2] is not None for r in base_rows)

        def statement(rows):
            want = None
            try:
                R.insert_stmt(shape, R.Store(shape, st.rows), rows, st.rowid_base)
            except R.KeyExists as e:
                want = e
            try:
                ex, out = run(ctx, pk, rows, 1024, st.store, st.rowid_base)
            except KeyExistsError as e:
                assert want is not None and (e.row, e.stream, e.dup_handle) == (want.row, want.stream, want.dup_handle)
                return e
            assert want is None
            return ex, out

        # no conflict: NULLs in unique columns repeat freely; the batches are the ones the executor hands out without a store
        ok = fresh_rows(3000)
        ok[5] = (ok[5][0], None, ok[5][2])
        ok[2005] = (ok[2005][0], None, None)
        ok[2006] = (ok[2006][0], 7, None)
        if not pk:
            ok = [(None,) + r[1:] for r in ok]
        ex, out = statement(ok)
        _, plain = run(ctx, pk, ok, 1024, None, st.rowid_base)
        assert ex.rowCount == 3000 and len(out) == 3 == len(plain)
        for a, b in zip(out, plain):
            assert a[0] == b[0] and (a[1] == b[1]).all() and (a[2] == b[2]).all() and bytes(a[3][0]) == bytes(b[3][0])
            for x, y in zip(a[4], b[4]):
                assert all(bytes(p) == bytes(q) for p, q in zip(x, y))
        # a stored entry met in the third chunk, on the LAST stream; an earlier stream's conflict in a later row does not matter
        rows = list(ok)
        rows[2100] = rows[2100][:2] + (b"s00021",)
        rows[2500] = (rows[2500][0], 3 * 50, rows[2500][2])
        e = statement(rows)
        assert (e.row, e.stream, e.from_store) == (2100, 2 if pk else 1, True)
        # inside the statement, across chunks: the entry of the FIRST row of the group
        rows = list(ok)
        rows[10] = (rows[10][0], 424242, rows[10][2])
        rows[1500] = (rows[1500][0], 424242, rows[1500][2])
        rows[2900] = (rows[2900][0], 424242, rows[2900][2])
        e = statement(rows)
        assert (e.row, e.stream, e.from_store, e.dup_row) == (1500, 1 if pk else 0, False, 10)
        assert e.dup_handle == (rows[10][0] if pk else st.rowid_base + 11)
        # the batches wait in HBM: a statement beyond max_rows is refused, the shim runs the Go operator
        with pytest.raises(_lib.TsqError, match="max_rows") as r:
            run(ctx, pk, ok, 1024, st.store, st.rowid_base, max_rows=2999)
        assert r.value.status == abi.ERR_UNSUPPORTED
        if pk:  # the handle itself: stored, and twice in the statement
            rows = list(ok)
            rows[1030] = (10 * 7,) + rows[1030][1:]
            e = statement(rows)
            assert (e.row, e.stream, e.dup_handle) == (1030, 0, 70)
            rows[1030] = rows[3]
            rows[1030] = (rows[3][0], rows[1030][1] + 5000000, b"other")
            e = statement(rows)
            assert (e.row, e.stream, e.from_store, e.dup_handle) == (1030, 0, False, rows[3][0])
    finally:
        st.close()
