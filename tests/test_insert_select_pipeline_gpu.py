"""GPU: DeviceTableScan -> GpuSelectionExec -> GpuInsertSelectExec — INSERT INTO t (c, a, b, d, e) SELECT .. WHERE .. with everything in
HBM — into a table (id BIGINT PRIMARY KEY AUTO_INCREMENT, a INT, b TINYINT UNSIGNED NOT NULL, c DOUBLE(8,2), d VARCHAR(8) utf8mb4, e CHAR(4))
with a unique index on (a) and a non-unique one on (b, d).  Every KV pair is compared with the oracle's rowcodec / index-key encoders
applied to the rows tests/cast_ref.py makes of the select's rows; the produced rows decode back through tableScanExec to the cast
values; a failing statement reports the row, the column and the kind of its first error."""
import numpy as np
import pytest

from tests import cast_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import coprocessor
from tinysql_amd import expression as E
from tinysql_amd import rowcodec as RC
from tinysql_amd import table as T
from tinysql_amd.chunk import Chunk, Column, StrColumn, concat
from tinysql_amd.gpu_pipeline import (DeviceChunk, DeviceTableScan, GpuInsertSelectExec, GpuSelectionExec, InsertIndexInfo, InsertTableInfo, drain_device)

pytestmark = pytest.mark.gpu

TABLE_ID = 45
FTS = [R.FieldType(abi.TP_LONGLONG, not_null=True, auto_increment=True), R.FieldType(abi.TP_LONG), R.FieldType(abi.TP_TINY, unsigned=True, not_null=True),
       R.FieldType(abi.TP_DOUBLE, 8, 2), R.FieldType(abi.TP_VARCHAR, 8, charset="utf8mb4"), R.FieldType(abi.TP_STRING, 4, charset="utf8mb4")]
COL_IDS = [1, 2, 3, 4, 5, 300]
INSERT_COLUMNS = [3, 1, 2, 4, 5]    # the statement names (c, a, b, d, e); the select yields (DOUBLE, BIGINT, BIGINT, string, string, BIGINT filter column)
SRC_COLS = [-1, 1, 2, 0, 3, 4]
SRC_TYPES = [abi.F64, abi.I64, abi.I64, abi.BYTES, abi.BYTES]
WORDS = [b"", b"a", b"ab ", b"abcd", b"abcdefgh", b"abcdefghi", "h\u00e9llo w\u00f6rld".encode(), "\u20ac\u20ac\u20ac\u20ac".encode(), "\U0001F600x".encode(), b"x\xffy", b"pad   ", "\u00e9\u00e9\u00e9\u00e9\u00e9".encode()]
N = 5000


def table_info():
    cols = [T.ColumnInfo(f.tp, f.flen, f.decimal, (T.UnsignedFlag if f.unsigned else 0) | (T.NotNullFlag if f.not_null else 0) |
                         (T.AutoIncrementFlag | T.PriKeyFlag if f.auto_increment else 0), DefaultValue=f.default, Charset=f.charset) for f in FTS]
    return InsertTableInfo(TABLE_ID, cols, COL_IDS, PKIsHandle=True, pk_offset=0)


INDICES = [InsertIndexInfo(7, True, [1]), InsertIndexInfo(8, False, [2, 4])]


def source(n=N, seed=3):
    rng = np.random.default_rng(seed)
    c = Column(abi.F64, np.round(rng.uniform(-2e6, 2e6, n), 4), rng.random(n) > 0.15)   # beyond DOUBLE(8,2) now and then
    a = Column(abi.I64, rng.integers(-(1 << 33), 1 << 33, n), rng.random(n) > 0.2)      # beyond INT now and then
    b = Column(abi.I64, rng.integers(-20, 300, n))                                       # beyond TINYINT UNSIGNED now and then
    d = StrColumn([None if rng.random() < 0.1 else WORDS[i] for i in rng.integers(0, len(WORDS), n)])   # beyond 8 runes, invalid bytes now and then
    e = StrColumn([None if rng.random() < 0.1 else WORDS[i] for i in rng.integers(0, len(WORDS), n)])   # beyond 4 runes, trailing spaces
    f = Column(abi.I64, rng.integers(0, 10, n))                                          # WHERE f < 7
    return Chunk([c, a, b, d, e, f])


def selected(chunk):
    keep = chunk.columns[5].data < 7
    rows = Chunk(chunk.columns[:5]).rows()
    return [list(rows[i]) for i in np.nonzero(keep)[0]]


def column_of(tp, vals, dtype=None):
    if tp == abi.BYTES:
        return StrColumn(vals)
    return Column(tp, np.array([0 if v is None else v for v in vals], dtype=dtype), np.array([v is not None for v in vals]))


def run_insert(ctx, chunk, stmt, batch_rows, autoid_base=100):
    dt = DeviceChunk.from_host(ctx, chunk)
    ex = None
    try:
        sel = GpuSelectionExec(ctx, DeviceTableScan(ctx, dt, batch_rows), [E.ScalarFunction("lt", E.Column(5, abi.I64), E.Constant(7))])
        ex = GpuInsertSelectExec(ctx, sel, table_info(), INSERT_COLUMNS, INDICES, stmt, autoid_base=autoid_base)
        ex.Open()
        out = []
        while True:
            b = ex.Next()
            if b is None:
                break
            try:
                out.append((b.rows.to_host(),) + b.to_host())
            finally:
                b.free()
        return ex, out
    finally:
        if ex is not None:
            ex.Close()
        dt.free()


def test_every_kv_pair_equals_the_oracle_on_cast_refs_rows(ctx, orc):
    chunk = source()
    flags = abi.CAST_IN_INSERT | abi.CAST_TRUNCATE_AS_WARNING
    rows, sc = R.cast_rows(flags, selected(chunk), SRC_TYPES, FTS, SRC_COLS)
    ids, new_base, first, last = R.fill_auto_ids([r[0] for r in rows], 100, False, R.I64MAX)
    for r, i in zip(rows, ids):
        r[0] = i
    ex, batches = run_insert(ctx, chunk, T.StatementContext(TruncateAsWarning=True), 1536)
    assert len(batches) > 2 and ex.rowCount == len(rows) and ex.rowCount > 3000
    assert (ex.autoid_base, ex.lastInsertID, ex.insertID) == (new_base, first, last) and first == 101
    assert (ex.warnings["overflow"], ex.warnings["bad_null"]) == (sc.warn_overflow, 0) and sc.warn_overflow > 100
    assert (ex.warnings["data_too_long"], ex.warnings["bad_utf8"]) == (sc.warn_too_long, sc.warn_bad_utf8) and sc.warn_too_long > 100 and sc.warn_bad_utf8 > 100
    types = [f.out_type() for f in FTS]
    got_rows = concat([b[0] for b in batches], types)
    assert got_rows.rows() == [tuple(r) for r in rows]
    # the KV pairs, batch by batch, against the oracle's encoders on the reference's rows
    at = 0
    all_keys, all_vals, all_offs = [], [], [0]
    for cast, keys, (vals, offs), idx in batches:
        n = cast.NumRows()
        want = Chunk([column_of(t, [r[c] for r in rows[at:at + n]], cast.columns[c].data.dtype) for c, t in enumerate(types)])
        handles = np.array(ids[at:at + n], dtype=np.int64)
        assert [bytes(k) for k in keys] == [orc.encode_row_key(TABLE_ID, int(h)) for h in handles]
        ovals, ooffs = orc.rowcodec_encode(Chunk(want.columns[1:]), COL_IDS[1:])  # the PK-handle column is not stored in the row
        assert bytes(vals) == bytes(ovals) and (offs == ooffs).all()
        for ix, (ik, iko, iv, ivo, dist) in zip(INDICES, idx):
            icols = Chunk([want.columns[c] for c in ix.Columns])
            has_null = np.array([None in r for r in icols.rows()])
            in_key = np.ones(n, np.uint8) if not ix.Unique else has_null.astype(np.uint8)
            ok, oko = orc.encode_index_keys(icols, TABLE_ID, ix.ID, handles, in_key)
            assert bytes(ik) == bytes(ok) and (iko == oko).all()
            assert (dist == (1 - in_key)).all()
            v = bytes(iv)
            for r in range(n):
                cell = v[ivo[r]:ivo[r + 1]]
                assert cell == (int(handles[r]).to_bytes(8, "big", signed=True) if dist[r] else b"0")
        all_keys.append(keys.reshape(-1))
        all_vals.append(vals)
        all_offs += (offs[1:] + all_offs[-1]).tolist()
        at += n
    # ... and back: the stored rows through tableScanExec give the cast values again
    infos = [RC.ColInfo(-1, RC.TypeLonglong, IsPKHandle=True), RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(3, RC.TypeTiny, Flag=RC.UnsignedFlag),
             RC.ColInfo(4, RC.TypeDouble), RC.ColInfo(5, RC.TypeVarchar), RC.ColInfo(300, RC.TypeString)]
    scan = coprocessor.tableScanExec(ctx, infos, np.concatenate(all_keys), np.concatenate(all_vals), np.array(all_offs, dtype=np.int64))
    back = [r for ch in drain_device(scan) for r in ch.rows()]
    assert back == [tuple(r) for r in rows]


def test_a_failing_statement_reports_row_column_and_code(ctx):
    chunk = source()
    picked = selected(chunk)
    strict = T.StatementContext()
    with pytest.raises(R.CastError) as w:
        R.cast_rows(abi.CAST_IN_INSERT, picked, SRC_TYPES, FTS, SRC_COLS)
    for batch_rows in (1536, 1 << 20):  # the failing row in a later batch / in the only batch: .row counts from the statement's start
        with pytest.raises(T.CastError) as e:
            run_insert(ctx, chunk, strict, batch_rows)
        assert (e.value.row, e.value.column, e.value.status) == (w.value.row, w.value.col, w.value.code)
    # a value beyond INT far behind the first rows (the third batch of 1024), none before it
    n = 3000
    late = np.arange(n)
    late[2100] = 1 << 31
    words = StrColumn([b"w%d" % (i % 90) for i in range(n)])
    far = Chunk([Column(abi.F64, np.arange(n) * 0.5), Column(abi.I64, late), Column(abi.I64, np.arange(n) % 200), words, words, Column(abi.I64, np.zeros(n, np.int64))])
    with pytest.raises(T.CastError) as e:
        run_insert(ctx, far, strict, 1024)
    assert (e.value.row, e.value.column, e.value.status) == (2100, 1, abi.ERR_OUT_OF_RANGE)
    # a NULL for the NOT NULL column b
    good = Chunk([Column(abi.F64, np.arange(n) * 0.5), Column(abi.I64, np.arange(n)), Column(abi.I64, np.arange(n) % 200, np.arange(n) != 2500), words, words,
                  Column(abi.I64, np.zeros(n, np.int64))])
    with pytest.raises(T.CastError) as e:
        run_insert(ctx, good, strict, 1024)
    assert (e.value.row, e.value.column, e.value.status) == (2500, 2, abi.ERR_BAD_NULL)
    # a VARCHAR(8) value of nine runes in the third batch, and an invalid byte for CHAR(4) behind it
    wl = [b"w%d" % (i % 90) for i in range(n)]
    wl[2222] = "\u00e9".encode() * 9
    bad_e = list(wl)
    bad_e[2222], bad_e[2300] = b"ok", b"a\xffb"
    for dcol, ecol, want in ((StrColumn(wl), words, (2222, 4, abi.ERR_DATA_TOO_LONG)), (words, StrColumn(bad_e), (2300, 5, abi.ERR_BAD_UTF8))):
        chk = Chunk([Column(abi.F64, np.arange(n) * 0.5), Column(abi.I64, np.arange(n)), Column(abi.I64, np.arange(n) % 200), dcol, ecol, Column(abi.I64, np.zeros(n, np.int64))])
        with pytest.raises(T.CastError) as e:
            run_insert(ctx, chk, strict, 1024)
        assert (e.value.row, e.value.column, e.value.status) == want
    # the ids leave BIGINT's range before that row: the allocator's error is the statement's
    with pytest.raises(T.AutoIDError) as e:
        run_insert(ctx, good, strict, 1024, autoid_base=R.I64MAX - 2100)
    assert e.value.status == abi.ERR_UNSUPPORTED


def test_no_auto_value_on_zero_and_explicit_ids_move_the_allocator_once(ctx):
    """the statement names id too: explicit ids, zeros and NULLs in one column"""
    n = 2600
    rng = np.random.default_rng(8)
    idv = [None if rng.random() < 0.5 else 0 if rng.random() < 0.3 else int(rng.integers(1, 9000)) for _ in range(n)]
    chunk = Chunk([Column(abi.I64, np.array([0 if v is None else v for v in idv]), np.array([v is not None for v in idv])), Column(abi.I64, np.arange(n) % 250)])
    info = InsertTableInfo(TABLE_ID, table_info().Columns[:1] + table_info().Columns[2:3], [1, 3], PKIsHandle=True, pk_offset=0)
    for no_zero in (False, True):
        want_ids, nb, first, last = R.fill_auto_ids(idv, 50, no_zero)
        dt = DeviceChunk.from_host(ctx, chunk)
        ex = GpuInsertSelectExec(ctx, DeviceTableScan(ctx, dt, 1024), info, [0, 1], [], T.StatementContext(NoAutoValueOnZero=no_zero), autoid_base=50)
        try:
            ex.Open()
            got = []
            while True:
                b = ex.Next()
                if b is None:
                    break
                try:
                    got += b.rows.to_host().columns[0].data.tolist()
                finally:
                    b.free()
        finally:
            ex.Close()
            dt.free()
        assert got == want_ids and (ex.autoid_base, ex.lastInsertID, ex.insertID) == (nb, first, last)
