"""The per-row step of INSERT .. SELECT above the C-ABI (include/tsq.h "INSERT .. SELECT"): table.CastValue on every cell
(table/column.go:142-189), the defaults of the columns the statement does not name, Column.HandleBadNull (:290-299) and the
auto-increment ids (executor/insert_common.go:594-638) — over host chunks or device chunks.  Host plumbing only: every cell is
computed by libtsq's kernels, the defaults included (a default is cast once, as a one-row chunk, when the handle is made).
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib
from .chunk import Chunk, Column, np_dtype

# mysql.*Flag (parser/mysql/type.go) as far as this step reads them
NotNullFlag, PriKeyFlag, UnsignedFlag, AutoIncrementFlag, PreventNullInsertFlag = 1, 2, 32, 512, 1 << 20
INT_TYPES = (abi.TP_TINY, abi.TP_SHORT, abi.TP_INT24, abi.TP_LONG, abi.TP_LONGLONG)
_INT_BITS = {abi.TP_TINY: 8, abi.TP_SHORT: 16, abi.TP_INT24: 24, abi.TP_LONG: 32, abi.TP_LONGLONG: 64}


class ColumnInfo:
    """model.ColumnInfo: FieldType (Tp, Flen, Decimal, Flag) + the default.  DefaultValue: None (DEFAULT NULL / no default), an
    int, a float, or bytes / str for a string column — the value before the cast, as model.ColumnInfo keeps it.  Charset: "binary",
    "utf8" (3-byte), "utf8mb4"; anything else counts bytes and has no UTF-8 check"""

    def __init__(self, Tp, Flen=-1, Decimal=-1, Flag=0, DefaultValue=None, Name="", Charset=""):
        self.Tp, self.Flen, self.Decimal, self.Flag, self.DefaultValue, self.Name, self.Charset = Tp, Flen, Decimal, Flag, DefaultValue, Name, Charset

    def cast_flags(self):
        f = 0
        if self.Flag & UnsignedFlag:
            f |= abi.CAST_UNSIGNED
        if self.Flag & (NotNullFlag | PreventNullInsertFlag):
            f |= abi.CAST_NOT_NULL
        if self.Flag & AutoIncrementFlag:
            f |= abi.CAST_AUTO_INCREMENT
        return f | {"binary": abi.CAST_CHARSET_BIN, "utf8": abi.CAST_CHARSET_UTF8, "utf8mb4": abi.CAST_CHARSET_UTF8MB4}.get(self.Charset, 0)

    def out_type(self):
        if self.Tp in INT_TYPES:
            return abi.U64 if self.Flag & UnsignedFlag else abi.I64
        if self.Tp == abi.TP_FLOAT:
            return abi.F32
        if self.Tp == abi.TP_DOUBLE:
            return abi.F64
        return abi.BYTES

    def upper_bound(self):
        """IntergerSignedUpperBound of an integer column"""
        return (1 << (_INT_BITS[self.Tp] - 1)) - 1


class StatementContext:
    """the bits of stmtctx.StatementContext / the SQL mode this step reads (executor/executor.go ResetContextOfStmt)"""

    def __init__(self, IgnoreTruncate=False, TruncateAsWarning=False, OverflowAsWarning=False, BadNullAsWarning=False, InInsertStmt=True,
                 SkipUTF8Check=False, NoAutoValueOnZero=False):
        self.IgnoreTruncate, self.TruncateAsWarning, self.OverflowAsWarning = IgnoreTruncate, TruncateAsWarning, OverflowAsWarning
        self.BadNullAsWarning, self.InInsertStmt, self.SkipUTF8Check, self.NoAutoValueOnZero = BadNullAsWarning, InInsertStmt, SkipUTF8Check, NoAutoValueOnZero

    def str_ctx(self):
        """the TSQ_STRCTX_* flags types.StrToInt / StrToUint read: an INSERT is neither a SELECT nor a DELETE and has CastStrToIntStrict off"""
        c = abi.STRCTX_NOT_STRICT | abi.STRCTX_EMPTY_NOT_ZERO
        if self.IgnoreTruncate:
            return c | abi.STRCTX_IGNORE_TRUNCATE
        return c if self.TruncateAsWarning else c | abi.STRCTX_TRUNCATE_ERROR

    def cast_flags(self):
        return ((abi.CAST_IGNORE_TRUNCATE if self.IgnoreTruncate else 0) | (abi.CAST_TRUNCATE_AS_WARNING if self.TruncateAsWarning else 0) |
                (abi.CAST_OVERFLOW_AS_WARNING if self.OverflowAsWarning else 0) | (abi.CAST_BAD_NULL_AS_WARNING if self.BadNullAsWarning else 0) |
                (abi.CAST_IN_INSERT if self.InInsertStmt else 0) | (abi.CAST_SKIP_UTF8_CHECK if self.SkipUTF8Check else 0))


class CastError(_lib.TsqError):
    """the first failing cell of a run, in the reference's order: .row, .column (table column), .status"""

    def __init__(self, status, message, row, column):
        super().__init__(status, message)
        self.row, self.column = row, column


def _bits(tp, v):
    return int(np.array([v], dtype=np_dtype(tp)).view(np.uint32 if tp == abi.F32 else np.uint64)[0])


class Caster:
    """a tsq_cast handle: colInfos = the table's columns (Table.Cols()); src_cols[c] = the column of the select's chunk that feeds table
    column c, -1 when the statement does not name it; src_types = the types of the select's chunk"""

    def __init__(self, ctx, colInfos, src_cols, src_types, stmt, _defaults=True):
        self.ctx, self.lib, self.colInfos, self.stmt = ctx, ctx.lib, list(colInfos), stmt
        self.out_types = [ci.out_type() for ci in self.colInfos]
        n = len(self.colInfos)
        self.n_in = len(src_types)
        self._keep = []
        spec = (abi.CastCol * n)()
        for c, ci in enumerate(self.colInfos):
            s = spec[c]
            s.src_col, s.tp, s.flen, s.decimal, s.flags = src_cols[c], ci.Tp, ci.Flen, ci.Decimal, ci.cast_flags()
            s.src_type = src_types[src_cols[c]] if src_cols[c] >= 0 else 0
            if src_cols[c] < 0 and not (ci.Flag & AutoIncrementFlag):
                d = self._default(ci) if _defaults else None
                if d is None:
                    s.flags |= abi.CAST_DEFAULT_NULL
                elif self.out_types[c] == abi.BYTES:
                    buf = C.create_string_buffer(bytes(d), max(len(d), 1))
                    self._keep.append(buf)
                    s.def_bytes, s.def_len = C.cast(buf, C.c_void_p), len(d)
                else:
                    s.def_bits = _bits(self.out_types[c], d)
        h = C.c_void_p()
        _lib.check(self.lib.tsq_cast_create(ctx.h, spec, n, stmt.cast_flags(), stmt.str_ctx(), C.byref(h)), ctx.h)
        self.h = h
        self.warnings = {"overflow": 0, "truncated": 0, "data_too_long": 0, "bad_null": 0, "bad_utf8": 0}

    def _default(self, ci):
        """GetColDefaultValue: the default cast like any other value (table/column.go:345-370), by the kernels, on a one-row chunk"""
        v = ci.DefaultValue
        if v is None:
            return None
        if isinstance(v, (bytes, str)):
            from .chunk import StrColumn
            tp, col = abi.BYTES, StrColumn([v])
        else:
            tp = abi.F64 if isinstance(v, float) else (abi.U64 if v > (1 << 63) - 1 else abi.I64)
            col = Column(tp, np.array([v], dtype=np_dtype(tp)))
        one = Caster(self.ctx, [ColumnInfo(ci.Tp, ci.Flen, ci.Decimal, ci.Flag & ~AutoIncrementFlag, Charset=ci.Charset)], [0], [tp], self.stmt, _defaults=False)
        try:
            return one.run(Chunk([col])).columns[0].values()[0]
        finally:
            one.close()

    def run(self, chunk, partial=False):
        """a host Chunk -> a host Chunk; a DeviceChunk -> a DeviceChunk the caller frees.  Raises CastError at the first failing cell;
        partial (device chunks): the error then carries the output chunk as .partial (the caller frees it) — the cells of the rows
        in front of the failing one are what a successful run would have written"""
        from .gpu_pipeline import DeviceChunk, DeviceColumn
        from .chunk import make_cols, out_buffers, chunk_from_buffers
        n = chunk.NumRows()
        keep = []
        dev = isinstance(chunk, DeviceChunk)
        nc = len(self.out_types)
        cap, need = (C.c_int64 * nc)(), (C.c_int64 * nc)()
        in_cols = chunk.cols() if dev else make_cols(chunk.columns, keep)
        out = bufs = None
        while True:  # a table with string columns: the first pass asks for their sizes (cap_bytes = 0 writes nothing)
            var_bytes = [int(b) for b in cap]
            if dev:
                if out:
                    for c in out:
                        c.free()
                out = [DeviceColumn(self.ctx, t, n, cap_bytes=var_bytes[i]) for i, t in enumerate(self.out_types)]
                out_cols = (abi.Col * nc)(*[c.col(n) for c in out])
            else:
                out_cols, bufs = out_buffers(self.out_types, n, keep, var_bytes=var_bytes)
            st = self.lib.tsq_cast_run(self.h, in_cols, self.n_in, n, out_cols, cap, need)
            if st == abi.ERR_INVALID and any(need[i] > cap[i] for i in range(nc)):
                for i in range(nc):
                    cap[i] = need[i]
                continue
            break
        if st != abi.OK:
            row, col = C.c_int64(-1), C.c_int32(-1)
            msg = _lib.last_error(self.h)
            at = st != abi.ERR_INVALID and self.lib.tsq_cast_error_at(self.h, C.byref(row), C.byref(col)) == abi.OK
            if dev and not (partial and at):
                for c in out:
                    c.free()
            if at:
                e = CastError(st, msg, row.value, col.value)
                e.partial = DeviceChunk(out, n) if dev and partial else None
                raise e
            raise _lib.TsqError(st, msg)
        w = [C.c_int64(0) for _ in range(5)]
        _lib.check(self.lib.tsq_cast_warnings(self.h, *[C.byref(x) for x in w]), self.h)
        for k, x in zip(("overflow", "truncated", "data_too_long", "bad_null", "bad_utf8"), w):
            self.warnings[k] += x.value
        if dev:
            return DeviceChunk(out, n)
        return chunk_from_buffers(self.out_types, bufs, n)

    def stats(self):
        r, l, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_cast_stats(self.h, C.byref(r), C.byref(l), C.byref(ms)), self.h)
        return {"rows": r.value, "launches": l.value, "kernel_ms": ms.value}

    def close(self):
        if self.h:
            self.lib.tsq_cast_destroy(self.h)
            self.h = None


def CastValue(ctx, chunk, colInfos, stmt, src_cols=None):
    """table.CastValue + fillRow over a whole chunk: -> (chunk of the table's columns, warning counts).  src_cols defaults to the
    statement naming every column of the table in order"""
    src_cols = list(range(len(colInfos))) if src_cols is None else src_cols
    c = Caster(ctx, colInfos, src_cols, chunk.types(), stmt)
    try:
        return c.run(chunk), dict(c.warnings)
    finally:
        c.close()


class AutoIDError(_lib.TsqError):
    def __init__(self, status, message, row):
        super().__init__(status, message)
        self.row = row


def FillAutoID(ctx, column, nrows, base, colInfo, stmt):
    """adjustAutoIncrementDatum over the cast output of the auto-increment column, in place: `column` is a host chunk.Column (returned
    anew) or a gpu_pipeline.DeviceColumn.  -> (column, new_base, lastInsertID, InsertID)"""
    lib = ctx.lib
    host = isinstance(column, Column)
    keep = []
    if host:
        data = column.data.copy()
        bm = np.concatenate([np.packbits(column.notnull if column.notnull is not None else np.ones(nrows, bool), bitorder="little"), np.zeros(8, np.uint8)])
        col = abi.Col()
        col.data, col.null_bitmap, col.length = data.ctypes.data_as(C.c_void_p), bm.ctypes.data_as(C.c_void_p), nrows
        col.elem_size, col.type, col.flags = 8, abi.I64, 0
        keep += [data, bm]
    else:
        col = column.col(nrows)
    nb, first, last, bad = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(-1)
    st = lib.tsq_autoid_fill(ctx.h, C.byref(col), nrows, base, abi.AUTOID_NO_AUTO_VALUE_ON_ZERO if stmt.NoAutoValueOnZero else 0, colInfo.upper_bound(),
                             C.byref(nb), C.byref(first), C.byref(last), C.byref(bad))
    if st != abi.OK:
        raise AutoIDError(st, _lib.last_error(ctx.h), bad.value)
    if host:
        column = Column(abi.I64, data)
    return column, nb.value, first.value, last.value
