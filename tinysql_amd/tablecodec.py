"""Mirror of package tablecodec's record-key functions for the harness (tablecodec/tablecodec.go): the keys of a table scan
<-> handles, computed on the GPU by libtsq (`tsq_rowkeys_decode` / `tsq_rowkeys_encode`, SURVEY.md §8 f rank 4), and the write side:
`EncodeRow` (tablecodec.go:129, `tsq_rowcodec_encode`) and `GenIndexKeys` (index.GenIndexKey + the value index.Create stores,
table/tables/index.go:161-244, `tsq_indexkeys_encode`).

    record key = 't' | EncodeInt(tableID) | "_r" | EncodeInt(handle)        RecordRowKeyLen = 19 bytes

The batch forms are what a scan uses: mocktikv's tableScanExec calls DecodeRowKey once per KV pair (store/mockstore/mocktikv/
executor.go:124-196); the handles then feed `rowcodec.ChunkDecoder` for the PK-handle column.  Errors are the reference's
("invalid key", tablecodec.go:237) and surface as `_lib.TsqError`.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib

RecordRowKeyLen = 19  # tablecodec.go:39-44


def EncodeRowKeysWithHandles(ctx, tableID, handles):
    """EncodeRowKeyWithHandle (tablecodec.go:65-70) of every handle: np.uint8 array of 19 * n bytes."""
    h = np.ascontiguousarray(handles, dtype=np.int64)
    out = np.zeros(max(h.size, 1) * RecordRowKeyLen, np.uint8)
    _lib.check(ctx.lib.tsq_rowkeys_encode(ctx.h, tableID, h.ctypes.data_as(C.c_void_p), h.size, 0, out.ctypes.data_as(C.c_void_p)), ctx.h)
    return out[:h.size * RecordRowKeyLen]


def EncodeRowKeyWithHandle(ctx, tableID, handle):
    return bytes(EncodeRowKeysWithHandles(ctx, tableID, [handle]))


def DecodeRowKeys(ctx, keys, key_offsets=None, want_table_ids=False):
    """DecodeRowKey (tablecodec.go:235-242) of every key of `keys` (bytes / np.uint8; 19-byte keys back to back, or cut by
    key_offsets[n + 1]).  Returns handles (and the table ids DecodeRecordKey hands back).  The first key in scan order that is
    not a record key raises TsqError("invalid key") — the scan ends there, as tableScanExec returns the error."""
    raw = np.frombuffer(keys, dtype=np.uint8) if isinstance(keys, (bytes, bytearray)) else np.ascontiguousarray(keys, dtype=np.uint8)
    offs = None if key_offsets is None else np.ascontiguousarray(key_offsets, dtype=np.int64)
    if offs is None and raw.size % RecordRowKeyLen:
        raise _lib.TsqError(abi.ERR_INVALID, "invalid key")  # a trailing partial key: len(key) != RecordRowKeyLen
    n = raw.size // RecordRowKeyLen if offs is None else len(offs) - 1
    handles = np.zeros(max(n, 1), np.int64)
    tids = np.zeros(max(n, 1), np.int64) if want_table_ids else None
    got = C.c_int64(0)
    buf = raw if raw.size else np.zeros(1, np.uint8)
    _lib.check(ctx.lib.tsq_rowkeys_decode(ctx.h, buf.ctypes.data_as(C.c_void_p), raw.size, None if offs is None else offs.ctypes.data_as(C.c_void_p), n, 0,
                                          handles.ctypes.data_as(C.c_void_p), None if tids is None else tids.ctypes.data_as(C.c_void_p), C.byref(got)), ctx.h)
    return (handles[:n], tids[:n]) if want_table_ids else handles[:n]


def DecodeRowKey(ctx, key):
    return int(DecodeRowKeys(ctx, key, key_offsets=[0, len(key)])[0])


def DecodeRecordKey(ctx, key):
    """(tableID, handle) — tablecodec.go:73-77"""
    h, t = DecodeRowKeys(ctx, key, key_offsets=[0, len(key)], want_table_ids=True)
    return int(t[0]), int(h[0])


def EncodeRow(ctx, chunk, colIDs):
    """tablecodec.EncodeRow (tablecodec.go:129-141) of every row of a chunk: rowcodec.Encoder.Encode."""
    from . import rowcodec
    return rowcodec.Encoder().Encode(ctx, chunk, colIDs)


class DeviceIndexKVs:
    """the index entries of a device chunk, in HBM: keys / key_offsets, values / value_offsets, distinct (one byte per row)"""

    def __init__(self, ctx, n, nbytes):
        self.ctx, self.n, self.nbytes = ctx, n, nbytes
        self.keys, self.key_offsets = ctx.alloc(max(nbytes, 1) + 64), ctx.alloc((n + 1) * 8 + 64)
        self.values, self.value_offsets = ctx.alloc(max(n, 1) * 8 + 64), ctx.alloc((n + 1) * 8 + 64)
        self.distinct = ctx.alloc(max(n, 1) + 64)

    def to_host(self):
        n = self.n
        keys, ko = np.zeros(max(self.nbytes, 1), np.uint8), np.zeros(n + 1, np.int64)
        vals, vo, dist = np.zeros(max(n, 1) * 8, np.uint8), np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.uint8)
        for h, d in ((keys, self.keys), (ko, self.key_offsets), (vals, self.values), (vo, self.value_offsets), (dist, self.distinct)):
            self.ctx.d2h(h, d)
        return keys[:self.nbytes], ko, vals[:vo[n]], vo, dist[:n]

    def free(self):
        for p in (self.keys, self.key_offsets, self.values, self.value_offsets, self.distinct):
            if p:
                self.ctx.free(p)
        self.keys = self.key_offsets = self.values = self.value_offsets = self.distinct = None


def GenIndexKeys(ctx, tableID, indexID, unique, chunk, handles, prefix_len=None, prefix_utf8=None):
    """index.GenIndexKey (table/tables/index.go:161-189) + the value index.Create stores (:224-244) for every row of `chunk` (its
    columns = the index columns, in index order).  A host Chunk with host handles -> (keys, key_offsets, values, value_offsets,
    distinct) as numpy arrays; a DeviceChunk with handles in HBM (a device pointer) -> a DeviceIndexKVs (the caller frees it).
    prefix_len[c] / prefix_utf8[c]: the index column's prefix length (-1: none) and whether it counts runes (a utf8 charset)."""
    from .rowcodec import chunk_cols
    keep = []
    cols, n, dev = chunk_cols(chunk, keep)
    nc = len(chunk.columns)
    pl = None if prefix_len is None else (C.c_int32 * nc)(*prefix_len)
    pu = None if prefix_utf8 is None else (C.c_uint8 * nc)(*[1 if u else 0 for u in prefix_utf8])
    fl = abi.IDX_UNIQUE if unique else 0
    if dev:
        hp = C.c_void_p(handles)
    else:
        h = np.ascontiguousarray(handles, dtype=np.int64)
        keep.append(h)
        hp = h.ctypes.data_as(C.c_void_p)
    need = C.c_int64(0)
    one = np.zeros(2, np.int64)  # the size question writes nothing, but the boundary arrays must be there
    st = ctx.lib.tsq_indexkeys_encode(ctx.h, tableID, indexID, fl, cols, nc, pl, pu, hp, n, 0, None, 0, one.ctypes.data_as(C.c_void_p), None,
                                      one.ctypes.data_as(C.c_void_p), None, C.byref(need))
    if st != abi.OK and not (st == abi.ERR_INVALID and need.value > 0):
        _lib.check(st, ctx.h)
    if dev:
        out = DeviceIndexKVs(ctx, n, need.value)
        try:
            _lib.check(ctx.lib.tsq_indexkeys_encode(ctx.h, tableID, indexID, fl, cols, nc, pl, pu, hp, n, abi.COL_DEVICE, C.c_void_p(out.keys), need.value,
                                                    C.c_void_p(out.key_offsets), C.c_void_p(out.values), C.c_void_p(out.value_offsets),
                                                    C.c_void_p(out.distinct), C.byref(need)), ctx.h)
        except Exception:
            out.free()
            raise
        return out
    keys, ko = np.zeros(max(need.value, 1), np.uint8), np.zeros(n + 1, np.int64)
    vals, vo, dist = np.zeros(max(n, 1) * 8, np.uint8), np.zeros(n + 1, np.int64), np.zeros(max(n, 1), np.uint8)
    _lib.check(ctx.lib.tsq_indexkeys_encode(ctx.h, tableID, indexID, fl, cols, nc, pl, pu, hp, n, 0, keys.ctypes.data_as(C.c_void_p), need.value,
                                            ko.ctypes.data_as(C.c_void_p), vals.ctypes.data_as(C.c_void_p), vo.ctypes.data_as(C.c_void_p),
                                            dist.ctypes.data_as(C.c_void_p), C.byref(need)), ctx.h)
    return keys[:need.value], ko, vals[:vo[n]], vo, dist[:n]
