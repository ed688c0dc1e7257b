"""Shared by the GPU tests of statements that go through the transaction buffer (INSERT .. SELECT into a table with secondary indexes,
DELETE .. WHERE): the table t (id BIGINT PRIMARY KEY as the handle, a BIGINT, s VARCHAR(16) NULL) with a non-unique index on a and a
unique index on s, the KV pairs of its rows from the oracle's encoders, stores built from them, and the scans that read a store back."""
import numpy as np

from tests import mvcc_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import coprocessor as cop
from tinysql_amd import rowcodec as RC
from tinysql_amd import table as T
from tinysql_amd.chunk import Chunk, Column, StrColumn
from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceTableScan, GpuInsertSelectExec, InsertIndexInfo, InsertTableInfo, drain_device

TID = 47
IDX_A, IDX_S = 1, 2
INDICES = [InsertIndexInfo(IDX_A, False, [1]), InsertIndexInfo(IDX_S, True, [2])]
SCAN_COLS = [RC.ColInfo(1, RC.TypeLonglong, 0, True), RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(3, RC.TypeVarchar)]  # (id, a, s): Table.Cols() order

flip = lambda v: ((int(v) + (1 << 63)) & ((1 << 64) - 1)).to_bytes(8, "big")
RECORD_PREFIX = b"t" + flip(TID) + b"_r"
index_prefix = lambda ix: b"t" + flip(TID) + b"_i" + flip(ix)


def table_info():
    cols = [T.ColumnInfo(abi.TP_LONGLONG, Flag=T.NotNullFlag | T.PriKeyFlag), T.ColumnInfo(abi.TP_LONGLONG), T.ColumnInfo(abi.TP_VARCHAR, 16, Charset="utf8mb4")]
    return InsertTableInfo(TID, cols, [1, 2, 3], PKIsHandle=True, pk_offset=0)


def make_rows(handles):
    """{handle: (a, s)}: a repeats (h mod 50), s is NULL for every 7th handle and unique otherwise"""
    return {int(h): (int(h) % 50, None if int(h) % 7 == 0 else b"s%07d" % (int(h) % 10000000)) for h in handles}


def rows_chunk(rows, order=None):
    hs = list(rows) if order is None else [int(h) for h in order]
    return Chunk([Column(abi.I64, np.array(hs, dtype=np.int64)), Column(abi.I64, np.array([rows[h][0] for h in hs], dtype=np.int64)),
                  StrColumn([rows[h][1] for h in hs])]), hs


def kv_pairs(orc, rows):
    """-> (record [(key, value)], index a [(key, value)], index s [(key, value)]) of the rows, from the oracle's encoders"""
    chunk, hs = rows_chunk(rows)
    n = len(hs)
    handles = np.array(hs, dtype=np.int64)
    vals, offs = orc.rowcodec_encode(Chunk(chunk.columns[1:]), [2, 3])
    raw = bytes(vals)
    rec = [(orc.encode_row_key(TID, h), raw[offs[i]:offs[i + 1]]) for i, h in enumerate(hs)]
    out = [rec]
    for ix, col in ((IDX_A, 1), (IDX_S, 2)):
        null = np.array([rows[h][col - 1] is None for h in hs])
        in_key = np.ones(n, np.uint8) if ix == IDX_A else null.astype(np.uint8)
        k, ko = orc.encode_index_keys(Chunk([chunk.columns[col]]), TID, ix, handles, in_key)
        k = bytes(k)
        out.append([(k[ko[i]:ko[i + 1]], b"0" if in_key[i] else int(h).to_bytes(8, "big", signed=True)) for i, h in enumerate(hs)])
    return tuple(out)


def committed_store(orc, rows, start_ts, commit_ts):
    s = R.Store()
    for stream in kv_pairs(orc, rows):
        for k, v in stream:
            s.versions[k] = [R.Value(R.PUT, start_ts, commit_ts, v)]
    return s


def read_back(ctx, ms, ts):
    """-> ({handle: (a, s)}, {(a, handle)} of index a, {(s, handle)} of index s) as the scans over the three ranges see the store at ts"""
    # (a range [p, PrefixNext(p)) has the shape of a point and would be read with Get: the ranges start one 0x00 behind the prefix)
    e = cop.tableScanExec.from_store(ctx, SCAN_COLS, ms, [(RECORD_PREFIX + b"\x00", cop.PrefixNext(RECORD_PREFIX))], ts)
    rows = {h: (a, s) for c in drain_device(e) for h, a, s in c.rows()}
    out = [rows]
    for ix, tp in ((IDX_A, abi.I64), (IDX_S, abi.BYTES)):
        p = index_prefix(ix)
        e = cop.indexScanExec.from_store(ctx, [tp, abi.I64], 1, cop.indexScanExec.PrimaryKeyIsSigned, ms, [(p + b"\x00", cop.PrefixNext(p))], ts, unique=(ix == IDX_S))
        got = [r for c in drain_device(e) for r in c.rows()]
        assert len(set(got)) == len(got)
        out.append(set(got))
    return tuple(out)


def expect_read(rows):
    return dict(rows), {(a, h) for h, (a, s) in rows.items()}, {(s, h) for h, (a, s) in rows.items()}


def insert_into(ctx, mb, rows, order, batch_rows=1024):
    """INSERT INTO t SELECT id, a, s in the given row order: every InsertBatch written to the buffer and freed -> batches seen"""
    chunk, _ = rows_chunk(rows, order)
    dt = DeviceChunk.from_host(ctx, chunk)
    ex = GpuInsertSelectExec(ctx, DeviceTableScan(ctx, dt, batch_rows), table_info(), [0, 1, 2], INDICES, T.StatementContext())
    seen = 0
    try:
        ex.Open()
        while True:
            bt = ex.Next()
            if bt is None:
                break
            try:
                bt.write_to(mb)
            finally:
                bt.free()
            seen += 1
    finally:
        ex.Close()
        dt.free()
    return seen


def model_sets(model, orc, rows):
    for stream in kv_pairs(orc, rows):
        for k, v in stream:
            model.Set(k, v)
