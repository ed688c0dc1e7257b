"""GPU: DeviceTableScan -> GpuReplaceSelectExec — REPLACE INTO t SELECT .. with everything in HBM, into a table with a primary key (or a
_tidb_rowid handle), two unique indexes and a plain one.  The store is what GpuInsertSelectExec wrote for an earlier statement, kept as
a dict of KV pairs; the ReplaceBatch is applied to that dict (deletions, then puts) and the dict must equal, byte for byte, the KV pairs
the oracle's encoders make of the final table of the SEQUENTIAL model (tests/dupcheck_ref.py: ReplaceExec.replaceRow line by line) —
record keys, stored rows, and the entries of every index.  Affected rows and the row-id base are the model's too."""
import numpy as np
import pytest

from tests import dupcheck_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import coprocessor
from tinysql_amd import table as T
from tinysql_amd.chunk import Chunk, concat
from tinysql_amd.gpu_pipeline import (DeviceChunk, DeviceTableScan, GpuInsertSelectExec, GpuReplaceSelectExec, InsertIndexInfo, InsertTableInfo)

pytestmark = pytest.mark.gpu

TABLE_ID = 41  # (the model's keys carry tests/dupcheck_ref.py's table id)
INDICES = [InsertIndexInfo(1, True, [1]), InsertIndexInfo(9, False, [1, 2]), InsertIndexInfo(2, True, [2])]  # unique (a), plain (a, s), unique (s)
TYPES = [abi.I64, abi.I64, abi.BYTES, abi.F64]
COL_IDS = [1, 2, 3, 4]
NAN = float("nan")


def table_info(pk, indexed_double=False):
    cols = [T.ColumnInfo(abi.TP_LONGLONG, Flag=(T.NotNullFlag | T.PriKeyFlag) if pk else 0), T.ColumnInfo(abi.TP_LONGLONG),
            T.ColumnInfo(abi.TP_VARCHAR, 80, Charset="utf8mb4"), T.ColumnInfo(abi.TP_DOUBLE)]
    return InsertTableInfo(TABLE_ID, cols, COL_IDS, PKIsHandle=pk, pk_offset=0 if pk else -1)


def shape_of(pk):
    return R.TableShape(TYPES, 0 if pk else None, [[(1, None)], [(2, None)]], TABLE_ID)


def kv_pairs(orc, pk, table):
    """{key bytes: value bytes} of a table {handle: row}: what tables.AddRecord writes for every row, by the oracle's encoders"""
    kv = {}
    items = sorted(table.items())
    if not items:
        return kv
    handles = np.array([h for h, _ in items], dtype=np.int64)
    chunk = R.chunk_of(TYPES, [r for _, r in items])
    stored = list(range(1 if pk else 0, len(TYPES)))  # the PK-handle column is not stored in the row
    vals, offs = orc.rowcodec_encode(Chunk([chunk.columns[c] for c in stored]), [COL_IDS[c] for c in stored])
    raw = bytes(vals)
    for k, h in enumerate(handles):
        kv[orc.encode_row_key(TABLE_ID, int(h))] = raw[offs[k]:offs[k + 1]]
    for ix in INDICES:
        icols = Chunk([chunk.columns[c] for c in ix.Columns])
        has_null = np.array([None in r for r in icols.rows()])
        in_key = has_null.astype(np.uint8) if ix.Unique else np.ones(len(items), np.uint8)
        ik, iko = orc.encode_index_keys(icols, TABLE_ID, ix.ID, handles, in_key)
        rawk = bytes(ik)
        for k, h in enumerate(handles):
            kv[rawk[iko[k]:iko[k + 1]]] = b"0" if in_key[k] else int(h).to_bytes(8, "big", signed=True)
    assert len(kv) == len(items) * (1 + len(INDICES))
    return kv


def batch_pairs(keys, vals_offs, idx):
    """the KV pairs of an InsertBatch.to_host()"""
    vals, offs = vals_offs
    raw = bytes(vals)
    out = [(bytes(k), raw[offs[r]:offs[r + 1]]) for r, k in enumerate(keys)]
    for ik, iko, iv, ivo, _ in idx:
        rk, rv = bytes(ik), bytes(iv)
        out += [(rk[iko[r]:iko[r + 1]], rv[ivo[r]:ivo[r + 1]]) for r in range(len(iko) - 1)]
    return out


class Stored:
    """the table an INSERT .. SELECT wrote: its KV pairs as a dict, and the storage side's device image of it"""

    def __init__(self, ctx, pk, rows):
        dt = DeviceChunk.from_host(ctx, R.chunk_of(TYPES, rows))
        ex = GpuInsertSelectExec(ctx, DeviceTableScan(ctx, dt, 1 << 20), table_info(pk), [0, 1, 2, 3], INDICES, T.StatementContext())
        try:
            ex.Open()
            b = ex.Next()
            try:
                hs = np.zeros(b.n, np.int64)
                ctx.d2h(hs, b.handles)
                got_rows = b.rows.to_host().rows()
                keys, (vals, offs), idx = b.to_host()
            finally:
                b.free()
        finally:
            ex.Close()
            dt.free()
        self.rows = list(zip(hs.tolist(), got_rows))
        self.rowid_base = 0 if pk else len(rows)
        self.kv = dict(batch_pairs(keys, (vals, offs), idx))
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


def replace(ctx, pk, st, rows, batch_rows, **kw):
    """-> (executor, the ReplaceBatch on the host: (deleted record keys, deleted index keys per index, puts), affected, rowid_base, n_removed)"""
    dt = DeviceChunk.from_host(ctx, R.chunk_of(TYPES, rows))
    ex = GpuReplaceSelectExec(ctx, DeviceTableScan(ctx, dt, batch_rows), table_info(pk), [0, 1, 2, 3], INDICES, T.StatementContext(), st.store,
                              rowid_base=st.rowid_base, **kw)
    try:
        ex.Open()
        b = ex.Next()
        try:
            host = b.to_host()
            out = (ex, host, b.affected, b.rowid_base, b.n_removed)
        finally:
            b.free()
        assert ex.Next() is None
        return out
    finally:
        ex.Close()
        dt.free()


def stored_rows(pk, m=400):
    """m rows; some with a NULL in a unique column (entries that are not distinct)"""
    return [(10 * k if pk else None, None if k % 17 == 0 else 3 * k, None if k % 13 == 0 else b"s%05d" % k, [0.0, 1.5, NAN, None][k % 4]) for k in range(m)]


def statement_rows(pk, base, n=3000, seed=4):
    """new rows, rows that meet stored rows on the handle, on (a), on (s), on several at once, stored rows again cell for cell (also with
    -0.0 for the stored 0.0: equal datums), earlier rows of the statement again, NULLs in the unique columns, string cells of 0..70 bytes"""
    rng = np.random.default_rng(seed)
    rows = []
    for r in range(n):
        x = rng.random()
        k = int(rng.integers(0, len(base)))
        b = base[k]
        if x < 0.08:
            row = b  # unchanged when the stored row is still there
        elif x < 0.12:
            row = b[:3] + (-0.0 if b[3] == 0.0 else b[3],)
        elif x < 0.2:
            row = (b[0], 100000 + r, b"n%07d" % r, 2.5)  # the handle (with a PK), other keys
        elif x < 0.28:
            row = (5000000 + r, b[1], b"n%07d" % r, 2.5)  # unique (a)
        elif x < 0.36:
            row = (5000000 + r, 100000 + r, b[2], 2.5)  # unique (s)
        elif x < 0.42:
            row = (5000000 + r, b[1], base[(k + 7) % len(base)][2], NAN)  # two stored rows at once
        elif x < 0.5 and rows:
            row = rows[int(rng.integers(0, len(rows)))]  # an earlier row of the statement again
        elif x < 0.56 and rows:
            e = rows[int(rng.integers(0, len(rows)))]
            row = (5000000 + r, e[1], b"m%07d" % r, 0.25)  # an earlier row's (a)
        elif x < 0.6:
            row = (5000000 + r, None, None if r % 2 else b"z" * (r % 71), None)
        else:
            row = (5000000 + r, 100000 + r, bytes([33 + (r * 7 + i) % 90 for i in range(r % 71)]) + b"%d" % r, float(r))
        rows.append(row if pk else (None,) + tuple(row[1:]))
    return rows


@pytest.mark.parametrize("pk", [True, False])
@pytest.mark.parametrize("batch_rows", [1024, 1 << 20])
def test_applied_batch_equals_the_models_kv_store_byte_for_byte(ctx, orc, pk, batch_rows):
    base = stored_rows(pk)
    st = Stored(ctx, pk, base)
    shape = shape_of(pk)
    try:
        assert st.kv == kv_pairs(orc, pk, dict(st.rows))  # the starting point is the oracle's too
        rows = statement_rows(pk, [r for _, r in st.rows])
        ex, (del_keys, del_idx, puts), affected, rowid_base, n_removed = replace(ctx, pk, st, rows, batch_rows)
        store = R.Store(shape, st.rows)
        want = R.replace_stmt(shape, store, rows, st.rowid_base)
        assert (affected, rowid_base, n_removed) == (want["affected"], want["rowid_base"], len(want["removed_store"]))
        assert want["added"].count(False) > 100 and want["n_removed_batch"] > 100 and len(want["removed_store"]) > 100  # the statement did collide
        kv = dict(st.kv)
        gone = [bytes(k) for k in del_keys]
        for ik, iko in del_idx:  # ALL index keys of the removed rows: every index, distinct entry or not
            raw = bytes(ik)
            assert len(iko) - 1 == n_removed
            gone += [raw[iko[r]:iko[r + 1]] for r in range(n_removed)]
        assert len(del_idx) == len(INDICES) and len(gone) == n_removed * (1 + len(INDICES)) == len(set(gone))
        for k in gone:
            del kv[k]  # (a KeyError: the batch deletes a pair the store does not hold)
        new = batch_pairs(*puts)
        assert len(new) == want["put"].count(True) * (1 + len(INDICES))
        for k, v in new:
            assert k not in kv, "a put over a live pair: its row was not deleted first"
            kv[k] = v
        assert kv == kv_pairs(orc, pk, store.table())
    finally:
        st.close()


def test_empty_statement_row_bound_and_float_index_refusals(ctx):
    st = Stored(ctx, True, stored_rows(True, 50))
    try:
        _, (del_keys, del_idx, puts), affected, _, n_removed = replace(ctx, True, st, [], 1024)
        assert (len(del_keys), del_idx, puts, affected, n_removed) == (0, [], None, 0, 0)
        rows = [(7000 + r, 7000 + r, b"q%d" % r, 1.0) for r in range(2100)]
        with pytest.raises(_lib.TsqError, match="max_rows") as e:
            replace(ctx, True, st, rows, 1024, max_rows=2000)
        assert e.value.status == abi.ERR_UNSUPPORTED
        _, _, affected, _, _ = replace(ctx, True, st, rows, 1024, max_rows=2100)
        assert affected == 2100
        with pytest.raises(_lib.TsqError, match="FLOAT / DOUBLE") as e:
            GpuReplaceSelectExec(ctx, None, table_info(True), [0, 1, 2, 3], [InsertIndexInfo(5, True, [3])], T.StatementContext(), st.store)
        assert e.value.status == abi.ERR_UNSUPPORTED
    finally:
        st.close()


@pytest.mark.parametrize("sizes", [(1,), (5, 3), (64, 1, 63, 1025), (1000, 1000, 1000, 4097)])
def test_device_chunk_append_equals_the_host_concatenation(ctx, sizes):
    rng = np.random.default_rng(sum(sizes))
    words = [None, b"", b"a", b"abcdefgh", b"abcdefghi", b"x" * 70]

    def part(m):
        return R.chunk_of(TYPES + [abi.BYTES], [(None if rng.random() < 0.2 else int(rng.integers(-9, 9)), int(rng.integers(0, 1 << 40)), words[int(rng.integers(0, 6))],
                                                 None if rng.random() < 0.3 else float(rng.integers(0, 5)), b"w%d" % int(rng.integers(0, 99))) for _ in range(m)])
    parts = [part(m) for m in sizes]
    dev = [DeviceChunk.from_host(ctx, p) for p in parts]
    # the destination owns its columns, each with a null bitmap (what the cast hands out)
    from tinysql_amd.gpu_pipeline import DeviceColumn
    acc = DeviceChunk([DeviceColumn(ctx, t, 4, cap_bytes=8 if t == abi.BYTES else 0) for t in TYPES + [abi.BYTES]], 0)
    try:
        for d in dev:
            acc.append(ctx, d)
        assert acc.NumRows() == sum(sizes)
        assert repr(acc.to_host().rows()) == repr(concat(parts, TYPES + [abi.BYTES]).rows())
    finally:
        acc.free()
        for d in dev:
            d.free()
