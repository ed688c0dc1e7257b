"""The storage side's coprocessor executors over libtsq — the harness mirror of store/mockstore/mocktikv's DAG handler
(cop_handler_dag.go:49-83 handleCopDAGRequest, :149-160 buildDAG), string columns included (SURVEY.md §8 f rank 4).

The reference runs the pushed-down plan row at a time over `[][]byte` datums: tableScanExec (executor.go:48-196: DecodeRowKey +
rowcodec.BytesDecoder.DecodeToBytes per KV pair) -> selectionExec (:322-390: decode the related columns, evalBool) -> hashAggExec
(aggregate.go:30-182: group key = EncodeValue of the group-by datums, aggregation.Aggregation.Update per row) | topNExec (:392-470 +
topn.go: a heap of `limit` rows) | limitExec (:472-507), then fillUpData4SelectResponse cuts the encoded rows into tipb.Chunks of 64
rows (cop_handler_dag.go:414-425, :510-519).  Here every executor is batch at a time and its chunks stay in HBM (gpu_pipeline.py's
device chunks); all compute runs in libtsq:
    tableScanExec  = tsq_rowkeys_decode (record keys -> handles) + tsq_rowcodec_decode (stored rows -> columns)
    indexScanExec  = tsq_indexkeys_decode (index keys [+ values] -> the index columns and the handle; memcomparable strings)
    tableLookupExec = tsq_lookup_task (a task's handles -> the rows of a DeviceTable that exist) + tsq_rows_gather (their stored rows,
                     back to back) + tsq_rowcodec_decode: the table worker's reader of IndexLookUpExecutor (executor/distsql.go:558-637)
    selectionExec  = tsq_filter_eval + tsq_chunk_compact
    hashAggExec    = tsq_agg_* in the partial layout of the reference: per function its partial results (AVG: count, sum —
                     avg.go:78-81), then the group-by values (aggregate.go:96-113)
    topNExec       = tsq_sort_* with a row limit (radix select + sort of the candidates)
    limitExec      = the first `limit` rows
    response       = tsq_rows_encode of the requested output offsets + the 64-row cut, or (encodeType "chunk") one wire chunk per
                     batch (tsq_chunk_encode), read back by chunk.Decoder
handleCopAnalyzeRequest (analyze.go:34-219) runs over the same two scans: handleAnalyzeColumnsReq = tableScanExec -> tsq_sorted_hist_* (the PK
handle) + tsq_analyze_* (the other columns); handleAnalyzeIndexReq = indexScanExec -> tsq_rows_encode (the key prefixes) -> tsq_analyze_*
(their CM sketch) + tsq_sorted_hist_* (the full key).
Same names and argument meaning as the reference's executors; differences that follow from running in parallel are the ones
DESIGN.md lists (group order, FIRST_ROW of a column that is not functionally dependent on the group key, the running-sum overflow).
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib
from . import rowcodec as RC
from .dupcheck import DevArray
from .executor import AggFuncDesc
from .gpu_pipeline import EOS, DeviceChunk, DeviceColumn, GpuExecutor, GpuHashAggExec, GpuSelectionExec, GpuSortExec
from .mvcc import ErrLocked

ROWS_PER_CHUNK = 64  # cop_handler_dag.go:510


class _DevBytes:
    """a byte / int64 array uploaded to HBM once"""

    def __init__(self, ctx, arr):
        self.ctx, self.n = ctx, arr.nbytes
        self.p = ctx.alloc(max(arr.nbytes, 1) + 64)
        if arr.nbytes:
            ctx.h2d(self.p, np.ascontiguousarray(arr))

    def free(self):
        if self.p:
            self.ctx.free(self.p)
            self.p = None


class _Sized:
    """the byte count of a buffer that lives in HBM only (what the scans read of raw_keys / raw_vals)"""

    def __init__(self, size):
        self.size = size


def PrefixNext(key):
    """kv.Key.PrefixNext: the smallest key greater than every key with this prefix"""
    b = bytearray(key)
    for i in range(len(b) - 1, -1, -1):
        b[i] = (b[i] + 1) & 0xFF
        if b[i] != 0:
            return bytes(b)
    return bytes(key) + b"\x00"


def storeRanges(kvRanges, desc, points=True):
    """the ranges of a scan as MvccStore.scan takes them.  points: a range with EndKey == StartKey.PrefixNext() is a point
    (kv.KeyRange.IsPoint) and is read with Get — what tableScanExec does for every such range (executor.go:124-137) and indexScanExec
    only for a UNIQUE index (`ran.IsPoint() && e.isUnique()`, executor.go:238, :270): the keys of a non-unique index carry the handle
    behind the indexed values, so [enc(v), PrefixNext(enc(v))) — the range of `WHERE col = v` — is scanned as the range it is.  A
    descending scan walks the ranges from the last to the first (reverseKVRanges, cop_handler_dag.go:477-509)"""
    rs = [(bytes(a), None) if points and bytes(b) == PrefixNext(bytes(a)) else (bytes(a), bytes(b)) for a, b in kvRanges]
    return rs[::-1] if desc else rs


class tableScanExec(GpuExecutor):
    """mocktikv.tableScanExec (executor.go:48-196) over the KV pairs of its ranges, in scan order: `keys` = the record keys back to
    back (19 bytes each), `values` / `value_offsets` = the stored rows (rowcodec v2).  columns: rowcodec.ColInfo of the scan's
    tipb.ColumnInfos (cop_handler_dag.go:162-208); a PK-handle column takes its value from the key (decoder.go:263-273)."""

    def __init__(self, ctx, columns, keys, values, value_offsets, batch_rows=1 << 22):
        self.columns = list(columns)
        types = [c.tsq_type() for c in self.columns]
        if any(t is None for t in types):
            raise _lib.TsqError(abi.ERR_UNSUPPORTED, "unknown type")  # a type the decoder does not know: the Go executors
        super().__init__(ctx, types)
        self.raw_keys = np.frombuffer(keys, dtype=np.uint8) if isinstance(keys, (bytes, bytearray)) else np.ascontiguousarray(keys, dtype=np.uint8)
        self.raw_vals = np.frombuffer(values, dtype=np.uint8) if isinstance(values, (bytes, bytearray)) else np.ascontiguousarray(values, dtype=np.uint8)
        self.offs = np.ascontiguousarray(value_offsets, dtype=np.int64)
        self.n = len(self.offs) - 1
        if self.raw_keys.size != 19 * self.n:
            raise _lib.TsqError(abi.ERR_INVALID, "invalid key")
        self.batch = (batch_rows + 7) & ~7
        self.rc = (abi.RowcodecCol * len(self.columns))()
        for i, c in enumerate(self.columns):
            self.rc[i].col_id, self.rc[i].type, self.rc[i].def_bits = c.ID, types[i], 0
            self.rc[i].flags = abi.RC_HANDLE if c.IsPKHandle else 0
            if c.Tp == RC.TypeBit:  # the stored uint as a binary literal of (Flen + 7) / 8 bytes (decoder.go:229-231)
                self.rc[i].flags |= abi.RC_BIT | (((c.Flen + 7) >> 3) << 8)
        self.dk = self.dv = self.do = self.dh = None
        self.out, self.pos, self.count = None, 0, 0

    @classmethod
    def from_store(cls, ctx, columns, store, kvRanges, startTS, desc=False, batch_rows=1 << 22):
        """the scan reading its pairs from an MvccStore at startTS (getRowFromRange / getRowFromPoint, executor.go:124-189): the pairs
        stay on the device, Counts() has one count per range — in scan order, i.e. reversed for desc.  A lock met by the read
        leaves Open as mvcc.ErrLocked."""
        e = _storeTableScanExec(ctx, columns, b"", b"", np.zeros(1, dtype=np.int64), batch_rows)
        e.read = (store, storeRanges(kvRanges, desc), startTS, desc)
        return e

    @classmethod
    def from_membuffer(cls, ctx, columns, membuf, kvRanges=None, desc=False, batch_rows=1 << 22, point_keys=None):
        """the scan reading its pairs from a finished kv.MemBuffer — the transaction's own writes (memTableReader, mem_reader.go:188-221):
        the PUT pairs of kvRanges in the order given, the whole sequence reversed for desc (tsq_membuf_scan); or, with point_keys =
        (device pointer to 19-byte record keys, n), the pairs of exactly those keys in their order (tsq_membuf_scan_points).  The
        pairs stay on the device."""
        e = _membufTableScanExec(ctx, columns, b"", b"", np.zeros(1, dtype=np.int64), batch_rows)
        if point_keys is not None:
            e.read = lambda: membuf.scan_points_packed(point_keys[0], None, 19 * point_keys[1], point_keys[1], device=True)
        else:
            e.read = lambda: membuf.scan([(bytes(a), bytes(b)) for a, b in kvRanges], desc, want_counts=True)
        return e

    def _load(self):
        ctx = self.ctx
        self.dk, self.dv, self.do = _DevBytes(ctx, self.raw_keys), _DevBytes(ctx, self.raw_vals), _DevBytes(ctx, self.offs)

    def Open(self):
        ctx = self.ctx
        self._load()
        self.dh = ctx.alloc(max(self.n, 1) * 8 + 64)
        # a string cell is a piece of its row: a var-len column of a batch cannot hold more bytes than the scanned values
        self.out = self._buffers(min(self.batch, max(self.n, 8)), var_bytes=[self.raw_vals.size] * len(self.types))
        self.pos = self.count = 0
        # DecodeRowKey of every pair (one launch for the whole scan: 27 bytes of traffic per row)
        got = C.c_int64(0)
        if self.n:
            _lib.check(self.lib.tsq_rowkeys_decode(ctx.h, C.c_void_p(self.dk.p), self.raw_keys.size, None, self.n, abi.COL_DEVICE, C.c_void_p(self.dh), None,
                                                   C.byref(got)), ctx.h)

    def Next(self):
        if self.pos >= self.n:
            return EOS
        lo, hi = self.pos, min(self.n, self.pos + self.batch)
        oc = (abi.Col * len(self.out))(*[c.col(hi - lo) for c in self.out])
        got = C.c_int64(0)
        # rows [lo, hi): their boundaries are offsets[lo .. hi] (absolute byte positions into `values`)
        _lib.check(self.lib.tsq_rowcodec_decode(self.ctx.h, C.c_void_p(self.dv.p), self.raw_vals.size, C.c_void_p(self.do.p + 8 * lo),
                                                C.c_void_p(self.dh + 8 * lo), hi - lo, abi.COL_DEVICE, len(self.columns), self.rc, oc, C.byref(got)), self.ctx.h)
        self.pos = hi
        self.count += got.value
        return DeviceChunk(self.out, got.value)

    def Counts(self):
        return [self.count]  # one range: rows handed on (executor.go:76-85)

    def Close(self):
        for b in (self.dk, self.dv, self.do):
            if b:
                b.free()
        if self.dh:
            self.ctx.free(self.dh)
        if self.out:
            for c in self.out:
                c.free()
        self.dk = self.dv = self.do = self.dh = self.out = None


class indexScanExec(GpuExecutor):
    """mocktikv.indexScanExec (executor.go:191-320) over the KV pairs of its ranges, in scan order: every pair through
    tablecodec.DecodeIndexKV (tablecodec.go:376-434).  `keys` / `key_offsets` = the index keys back to back; `values` /
    `value_offsets` = the pairs' values (the handle of a unique index, 8 bytes big endian); `types` = the index columns' types
    (+ the handle column, I64 or U64, when pkStatus != PrimaryKeyNotExists); colsLen = len(IndexScan.Columns) without the handle."""

    PrimaryKeyNotExists, PrimaryKeyIsSigned, PrimaryKeyIsUnsigned = 0, 1, 2  # tablecodec.go:394-403

    def __init__(self, ctx, types, colsLen, pkStatus, keys, key_offsets, values=b"", value_offsets=None, batch_rows=1 << 22):
        super().__init__(ctx, list(types))
        assert len(self.types) == colsLen + (1 if pkStatus else 0)
        self.colsLen, self.pkStatus = colsLen, pkStatus
        self.raw_keys = np.frombuffer(bytes(keys), dtype=np.uint8) if isinstance(keys, (bytes, bytearray)) else np.ascontiguousarray(keys, dtype=np.uint8)
        self.koffs = np.ascontiguousarray(key_offsets, dtype=np.int64)
        self.n = len(self.koffs) - 1
        self.raw_vals = np.frombuffer(bytes(values), dtype=np.uint8) if isinstance(values, (bytes, bytearray)) else np.ascontiguousarray(values, dtype=np.uint8)
        self.voffs = None if value_offsets is None else np.ascontiguousarray(value_offsets, dtype=np.int64)
        self.batch = batch_rows
        self.dk = self.dko = self.dv = self.dvo = None
        self.out, self.pos, self.count = None, 0, 0

    @classmethod
    def from_store(cls, ctx, types, colsLen, pkStatus, store, kvRanges, startTS, desc=False, batch_rows=1 << 22, unique=False):
        """the scan reading its pairs (keys and values) from an MvccStore at startTS, as tableScanExec.from_store does.  unique =
        IndexScan.Unique: only then is a point-shaped range read with Get (getRowFromPoint "is only used for unique key",
        executor.go:238, :270); on a non-unique index every range is scanned"""
        e = _storeIndexScanExec(ctx, types, colsLen, pkStatus, b"", np.zeros(1, dtype=np.int64), b"", np.zeros(1, dtype=np.int64), batch_rows)
        e.read = (store, storeRanges(kvRanges, desc, points=bool(unique)), startTS, desc)
        return e

    @classmethod
    def from_membuffer(cls, ctx, types, colsLen, pkStatus, membuf, kvRanges, desc=False, batch_rows=1 << 22):
        """the scan reading its pairs (keys and values) from a finished kv.MemBuffer, as tableScanExec.from_membuffer does
        (memIndexReader, mem_reader.go:67-130)"""
        e = _membufIndexScanExec(ctx, types, colsLen, pkStatus, b"", np.zeros(1, dtype=np.int64), b"", np.zeros(1, dtype=np.int64), batch_rows)
        e.read = lambda: membuf.scan([(bytes(a), bytes(b)) for a, b in kvRanges], desc, want_counts=True)
        return e

    def _load(self):
        ctx = self.ctx
        self.dk, self.dko = _DevBytes(ctx, self.raw_keys), _DevBytes(ctx, self.koffs)
        if self.voffs is not None:
            self.dv, self.dvo = _DevBytes(ctx, self.raw_vals), _DevBytes(ctx, self.voffs)

    def Open(self):
        ctx = self.ctx
        self._load()
        self.out = self._buffers(min(self.batch, max(self.n, 8)), var_bytes=[self.raw_keys.size] * len(self.types))  # a string cell is a piece of its key
        self.pos = self.count = 0

    def Next(self):
        if self.pos >= self.n:
            return EOS
        lo, hi = self.pos, min(self.n, self.pos + self.batch)
        oc = (abi.Col * len(self.out))(*[c.col(hi - lo) for c in self.out])
        tp = (C.c_int32 * len(self.types))(*self.types)
        got = C.c_int64(0)
        # pairs [lo, hi): their boundaries are key_offsets[lo .. hi] / value_offsets[lo .. hi] (absolute byte positions)
        _lib.check(self.lib.tsq_indexkeys_decode(self.ctx.h, C.c_void_p(self.dk.p), self.raw_keys.size, C.c_void_p(self.dko.p + 8 * lo), hi - lo,
                                                 C.c_void_p(self.dv.p) if self.dv else None, self.raw_vals.size if self.dv else 0,
                                                 C.c_void_p(self.dvo.p + 8 * lo) if self.dvo else None, abi.COL_DEVICE, self.colsLen, tp, self.pkStatus, oc,
                                                 C.byref(got)), self.ctx.h)
        self.pos = hi
        self.count += got.value
        return DeviceChunk(self.out, got.value)

    def Counts(self):
        return [self.count]

    def Close(self):
        for b in (self.dk, self.dko, self.dv, self.dvo):
            if b:
                b.free()
        if self.out:
            for c in self.out:
                c.free()
        self.dk = self.dko = self.dv = self.dvo = self.out = None


class _storeTableScanExec(tableScanExec):
    """tableScanExec.from_store: Open reads the ranges from the store (tsq_mvcc_scan + tsq_mvcc_fetch); everything behind is the parent's"""

    def _load(self):
        store, ranges, ts, desc = self.read
        pairs = store.scan(ranges, ts, desc)  # raises ErrLocked
        self.dk, self.dv, self.do, self.dko = pairs.keys, pairs.values, pairs.value_offsets, pairs.key_offsets
        self.n, self.raw_keys, self.raw_vals, self.range_counts = pairs.n, _Sized(pairs.key_bytes), _Sized(pairs.value_bytes), list(pairs.counts)
        if pairs.key_bytes != 19 * pairs.n:
            raise _lib.TsqError(abi.ERR_INVALID, "invalid key")

    def Counts(self):
        return list(self.range_counts)  # one count per range (executor.go:76-85)

    def Close(self):
        if getattr(self, "dko", None):
            self.dko.free()
            self.dko = None
        tableScanExec.Close(self)


class _storeIndexScanExec(indexScanExec):
    """indexScanExec.from_store"""

    def _load(self):
        store, ranges, ts, desc = self.read
        pairs = store.scan(ranges, ts, desc)  # raises ErrLocked
        self.dk, self.dko, self.dv, self.dvo = pairs.keys, pairs.key_offsets, pairs.values, pairs.value_offsets
        self.n, self.raw_keys, self.raw_vals, self.range_counts = pairs.n, _Sized(pairs.key_bytes), _Sized(pairs.value_bytes), list(pairs.counts)

    def Counts(self):
        return list(self.range_counts)


class _membufTableScanExec(_storeTableScanExec):
    """tableScanExec.from_membuffer: Open reads the pairs from the transaction buffer (tsq_membuf_scan / _scan_points + tsq_membuf_fetch)"""

    def _load(self):
        pairs = self.read()
        self.dk, self.dv, self.do, self.dko = pairs.keys, pairs.values, pairs.value_offsets, pairs.key_offsets
        self.n, self.raw_keys, self.raw_vals, self.range_counts = pairs.n, _Sized(pairs.key_bytes), _Sized(pairs.value_bytes), list(pairs.counts or [])
        if pairs.key_bytes != 19 * pairs.n:
            raise _lib.TsqError(abi.ERR_INVALID, "invalid key")


class _membufIndexScanExec(_storeIndexScanExec):
    """indexScanExec.from_membuffer"""

    def _load(self):
        pairs = self.read()
        self.dk, self.dko, self.dv, self.dvo = pairs.keys, pairs.key_offsets, pairs.values, pairs.value_offsets
        self.n, self.raw_keys, self.raw_vals, self.range_counts = pairs.n, _Sized(pairs.key_bytes), _Sized(pairs.value_bytes), list(pairs.counts or [])


class DeviceTable:
    """a table's KV pairs in scan order, uploaded once: the region in HBM every lookup task reads.  `keys` = the record keys back to
    back (19 bytes each), `values` / `value_offsets` = the stored rows (rowcodec v2), as tableScanExec takes them.  Holds the decoded
    handles (tsq_rowkeys_decode) and a tsq_lookup handle over them; record keys that are not in ascending handle order are refused
    ("table handles not ascending")."""

    def __init__(self, ctx, keys, values, value_offsets):
        self.ctx, self.lib = ctx, ctx.lib
        raw_keys = np.frombuffer(keys, dtype=np.uint8) if isinstance(keys, (bytes, bytearray)) else np.ascontiguousarray(keys, dtype=np.uint8)
        raw_vals = np.frombuffer(values, dtype=np.uint8) if isinstance(values, (bytes, bytearray)) else np.ascontiguousarray(values, dtype=np.uint8)
        offs = np.ascontiguousarray(value_offsets, dtype=np.int64)
        self.n, self.n_bytes = len(offs) - 1, raw_vals.size
        if raw_keys.size != 19 * self.n:
            raise _lib.TsqError(abi.ERR_INVALID, "invalid key")
        self.dv = self.do = self.dh = self.h = None
        dk = _DevBytes(ctx, raw_keys)
        try:
            self.dv, self.do = DevArray(ctx, raw_vals), DevArray(ctx, offs)  # (the type Pairs holds: from_pairs takes those over)
            self.dh = ctx.alloc(max(self.n, 1) * 8 + 64)
            got = C.c_int64(0)
            if self.n:
                _lib.check(self.lib.tsq_rowkeys_decode(ctx.h, C.c_void_p(dk.p), raw_keys.size, None, self.n, abi.COL_DEVICE, C.c_void_p(self.dh), None, C.byref(got)),
                           ctx.h)
            h = C.c_void_p()
            _lib.check(self.lib.tsq_lookup_create(ctx.h, C.c_void_p(self.dh), self.n, abi.COL_DEVICE, C.byref(h)), ctx.h)
            self.h = h
        except Exception:
            self.close()
            raise
        finally:
            dk.free()

    @classmethod
    def from_pairs(cls, ctx, pairs):
        """the table from device-resident fetched pairs (mvcc.Pairs: what tsq_mvcc_fetch, tsq_membuf_fetch and tsq_unionstore_fetch write)
        with no host round trip: the record keys are decoded where they lie, the stored rows and their offsets are KEPT — the table takes
        `pairs` over and frees the rest of it.  The pairs must be one table's records in ascending key order."""
        self = cls.__new__(cls)
        self.ctx, self.lib = ctx, ctx.lib
        self.n, self.n_bytes = pairs.n, pairs.value_bytes
        self.dv = self.do = self.dh = self.h = None
        try:
            if pairs.key_bytes != 19 * self.n:
                raise _lib.TsqError(abi.ERR_INVALID, "invalid key")
            self.dh = ctx.alloc(max(self.n, 1) * 8 + 64)
            got = C.c_int64(0)
            if self.n:
                _lib.check(self.lib.tsq_rowkeys_decode(ctx.h, C.c_void_p(pairs.keys.p), pairs.key_bytes, None, self.n, abi.COL_DEVICE, C.c_void_p(self.dh), None,
                                                       C.byref(got)), ctx.h)
            h = C.c_void_p()
            _lib.check(self.lib.tsq_lookup_create(ctx.h, C.c_void_p(self.dh), self.n, abi.COL_DEVICE, C.byref(h)), ctx.h)
            self.h = h
            self.dv, self.do = pairs.release_values()
        except Exception:
            self.close()
            raise
        finally:
            pairs.free()
        return self

    @classmethod
    def from_union(cls, us, table_id):
        """the table as the transaction sees it: one scan of the record range ['t' | id | "_r", 't' | id | "_s") through a kv.UnionStore —
        the committed rows under the transaction's own inserts, updates and deletes — then from_pairs; nothing leaves the device"""
        t = b"t" + ((int(table_id) + (1 << 63)) & ((1 << 64) - 1)).to_bytes(8, "big")
        return cls.from_pairs(us.ctx, us.scan([(t + b"_r", t + b"_s")]))

    def handles(self):
        """(device pointer to the table's handles in scan order, their number): what a HANDLE stream of the duplicate-key checker takes"""
        return self.dh, self.n

    def stats(self):
        a, b, c, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_lookup_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(ms)), self.h)
        return {"tasks": a.value, "handles": b.value, "found": c.value, "kernel_ms": ms.value}

    def close(self):
        if self.h:
            self.lib.tsq_lookup_destroy(self.h)
            self.h = None
        for b in (self.dv, self.do):
            if b:
                b.free()
        if self.dh:
            self.ctx.free(self.dh)
        self.dv = self.do = self.dh = None


class DeviceIndex:
    """a UNIQUE index's KV pairs in scan order, as indexScanExec takes them (keys / key_offsets, values / value_offsets), uploaded once:
    the DISTINCT entries — the ones whose value is the 8-byte big-endian handle (index.Create, table/tables/index.go:224-244; an entry
    with a NULL cell carries its handle in the key and the value "0") — with their decoded handles, in key order: what an INDEX stream
    of the duplicate-key checker (dupcheck.DupChecker) takes.  The cut is host plumbing on the arrays the caller hands over."""

    def __init__(self, ctx, keys, key_offsets, values, value_offsets):
        self.ctx = ctx
        raw_keys = np.frombuffer(keys, dtype=np.uint8) if isinstance(keys, (bytes, bytearray)) else np.ascontiguousarray(keys, dtype=np.uint8)
        raw_vals = np.frombuffer(values, dtype=np.uint8) if isinstance(values, (bytes, bytearray)) else np.ascontiguousarray(values, dtype=np.uint8)
        ko, vo = np.ascontiguousarray(key_offsets, dtype=np.int64), np.ascontiguousarray(value_offsets, dtype=np.int64)
        if len(ko) != len(vo) or len(ko) < 1:
            raise _lib.TsqError(abi.ERR_INVALID, "index keys and values differ in number")
        pick = np.nonzero(np.diff(vo) == 8)[0]
        lens = (ko[1:] - ko[:-1])[pick]
        offs = np.zeros(len(pick) + 1, np.int64)
        np.cumsum(lens, out=offs[1:])
        src = np.repeat(ko[:-1][pick] - offs[:-1], lens) + np.arange(int(offs[-1]), dtype=np.int64)
        hidx = (vo[:-1][pick][:, None] + np.arange(8)[None, :]).reshape(-1)
        handles = raw_vals[hidx].reshape(-1, 8)[:, ::-1].copy().view(np.int64).reshape(-1) if len(pick) else np.zeros(0, np.int64)
        self.n, self.key_bytes = len(pick), int(offs[-1])
        self.keys = self.key_offsets = self.handles = None
        try:
            self.keys = _DevBytes(ctx, raw_keys[src] if self.key_bytes else np.zeros(1, np.uint8))
            self.key_offsets = _DevBytes(ctx, offs)
            self.handles = _DevBytes(ctx, handles if self.n else np.zeros(1, np.int64))
        except Exception:
            self.close()
            raise

    @classmethod
    def from_union(cls, us, table_id, index_id):
        """the index as the transaction sees it: one scan of ['t' | table id | "_i" | index id, its PrefixNext) through a kv.UnionStore.
        The pairs are DOWNLOADED and go through the constructor above: the cut of the distinct entries is host plumbing today (DESIGN.md
        §8), so this side of the union read takes one round trip through the host."""
        flip = lambda v: ((int(v) + (1 << 63)) & ((1 << 64) - 1)).to_bytes(8, "big")
        prefix = b"t" + flip(table_id) + b"_i" + flip(index_id)
        p = us.scan([(prefix, PrefixNext(prefix))])
        try:
            ko, vo = p.key_offsets.read(np.int64, p.n + 1), p.value_offsets.read(np.int64, p.n + 1)
            return cls(us.ctx, p.keys.read(np.uint8, p.key_bytes), ko, p.values.read(np.uint8, p.value_bytes), vo)
        finally:
            p.free()

    def close(self):
        for b in (self.keys, self.key_offsets, self.handles):
            if b:
                b.free()
        self.keys = self.key_offsets = self.handles = None


class tableLookupExec(GpuExecutor):
    """the storage side of ONE task of IndexLookUpExecutor's table worker (executor/distsql.go:601-637: a table reader over the task's
    handles): tsq_lookup_task (handles -> row ordinals + handles of the rows that exist, ascending handle order or, with keep_order,
    the task's order), tsq_rows_gather (their stored rows, back to back) and tsq_rowcodec_decode for the scan's ColInfos.  The task's
    handles are a device array (set_task); Next hands out the task's rows as one device chunk, then the end.  The executor is
    re-armed by the next set_task; its buffers grow to the largest task and stay."""

    def __init__(self, ctx, table, columns, keep_order, handles=None, n=0):
        self.columns = list(columns)
        types = [c.tsq_type() for c in self.columns]
        if any(t is None for t in types):
            raise _lib.TsqError(abi.ERR_UNSUPPORTED, "unknown type")
        super().__init__(ctx, types)
        self.table, self.keep_order = table, 1 if keep_order else 0
        self.rc = (abi.RowcodecCol * len(self.columns))()
        for i, c in enumerate(self.columns):
            self.rc[i].col_id, self.rc[i].type, self.rc[i].def_bits = c.ID, types[i], 0
            self.rc[i].flags = abi.RC_HANDLE if c.IsPKHandle else 0
            if c.Tp == RC.TypeBit:
                self.rc[i].flags |= abi.RC_BIT | (((c.Flen + 7) >> 3) << 8)
        self.cap = self.cap_bytes = 0
        self.rows = self.hs = self.goffs = self.gvals = self.out = None
        self.count = 0
        self.set_task(handles, n)

    def set_task(self, handles, n):
        """handles: device pointer to n int64 handles in index-scan order"""
        self.task, self.task_n, self.done = handles, int(n), False

    def _grow(self, n):
        if n <= self.cap:
            return
        self._release_rows()
        self.cap = n
        self.rows, self.hs = self.ctx.alloc(n * 8 + 64), self.ctx.alloc(n * 8 + 64)
        self.goffs = self.ctx.alloc((n + 1) * 8 + 64)
        self.out = self._buffers(n)

    def Next(self):
        if self.done or self.task_n == 0:
            return EOS
        self.done = True
        ctx, lib, t, n = self.ctx, self.lib, self.table, self.task_n
        self._grow(n)
        nf = C.c_int64(0)
        _lib.check(lib.tsq_lookup_task(t.h, C.c_void_p(self.task), n, abi.COL_DEVICE, self.keep_order, C.c_void_p(self.rows), C.c_void_p(self.hs), C.byref(nf)), t.h)
        m = nf.value
        if m == 0:
            return EOS
        need = C.c_int64(0)
        args = (ctx.h, C.c_void_p(t.dv.p), t.n_bytes, C.c_void_p(t.do.p), t.n, C.c_void_p(self.rows), m)
        st = lib.tsq_rows_gather(*args, None, 0, None, C.byref(need))  # (asks for the size)
        if st != abi.OK and not (st == abi.ERR_INVALID and need.value > 0):
            _lib.check(st, ctx.h)
        if need.value > self.cap_bytes:
            if self.gvals:
                ctx.free(self.gvals)
            self.cap_bytes = int(need.value * 1.25) + 64
            self.gvals = ctx.alloc(self.cap_bytes + 64)
        if not self.gvals:
            self.gvals = ctx.alloc(64)
        _lib.check(lib.tsq_rows_gather(*args, C.c_void_p(self.gvals), need.value, C.c_void_p(self.goffs), C.byref(need)), ctx.h)
        for c in self.out:  # a string cell is a piece of its row
            c.ensure_bytes(need.value)
        oc = (abi.Col * len(self.out))(*[c.col(m) for c in self.out])
        got = C.c_int64(0)
        _lib.check(lib.tsq_rowcodec_decode(ctx.h, C.c_void_p(self.gvals), need.value, C.c_void_p(self.goffs), C.c_void_p(self.hs), m, abi.COL_DEVICE, len(self.columns),
                                           self.rc, oc, C.byref(got)), ctx.h)
        self.count += got.value
        return DeviceChunk(self.out, got.value)

    def Counts(self):
        return [self.count]

    def _release_rows(self):
        for p in (self.rows, self.hs, self.goffs):
            if p:
                self.ctx.free(p)
        if self.out:
            for c in self.out:
                c.free()
        self.rows = self.hs = self.goffs = self.out = None
        self.cap = 0

    def Close(self):
        self._release_rows()
        if self.gvals:
            self.ctx.free(self.gvals)
        self.gvals, self.cap_bytes = None, 0


class selectionExec(GpuSelectionExec):
    """mocktikv.selectionExec (executor.go:322-390): rows for which every condition is true (evalBool: NULL and 0 drop the row)."""

    def __init__(self, ctx, src, conditions):
        super().__init__(ctx, src, conditions)


class hashAggExec(GpuHashAggExec):
    """mocktikv.hashAggExec (aggregate.go:30-182).  aggFuncs: [(TSQ_AGG_*, argument column | -1 for the constant of COUNT(*))];
    groupByCols: bare columns (group-by EXPRESSIONS are evaluated by a projection below, as the planner does for the SQL side).
    Output row = partial results of every function in order, then the group-by values."""

    def __init__(self, ctx, src, aggFuncs, groupByCols, est_groups=0):
        in_types = src.Schema()
        descs = []
        for func, arg in aggFuncs:
            at = in_types[arg] if arg >= 0 else abi.I64
            # only AVG has a partial form that differs from its result (count, sum)
            descs.append(AggFuncDesc(func, arg, at, abi.MODE_PARTIAL1 if func == abi.AGG_AVG else abi.MODE_COMPLETE))
        for g in groupByCols:
            descs.append(AggFuncDesc(abi.AGG_FIRSTROW, g, in_types[g]))  # the group-by datum of the row that made the group
        super().__init__(ctx, src, list(groupByCols), descs, est_groups=est_groups)


class topNExec(GpuSortExec):
    """mocktikv.topNExec (executor.go:392-470, topn.go): the `limit` smallest rows under the ORDER BY items, in that order."""

    def __init__(self, ctx, src, orderByCols, desc, limit):
        super().__init__(ctx, src, list(orderByCols), list(desc), offset=0, count=limit)


class limitExec(GpuExecutor):
    """mocktikv.limitExec (executor.go:472-507): the first `limit` rows of its source, in the source's order."""

    def __init__(self, ctx, src, limit):
        super().__init__(ctx, src.Schema(), (src,))
        self.src, self.limit, self.cursor = src, int(limit), 0

    def Open(self):
        super().Open()
        self.cursor = 0

    def Next(self):
        if self.cursor >= self.limit:
            return EOS
        chk = self.src.Next()
        n = min(chk.NumRows(), self.limit - self.cursor)
        self.cursor += n
        return DeviceChunk(chk.columns, n) if n else EOS


def fillUpData4SelectResponse(ctx, chunk, outputOffsets, chunks=None, rowCnt=0):
    """cop_handler_dag.go:414-425 + appendRow :512-519: the requested columns of every row, encoded value by value
    (codec.EncodeValue) on the GPU, appended to `chunks` — RowsData pieces of 64 rows, a new piece whenever the running row count
    is a multiple of 64, whatever batches the rows arrive in.  chunk: a DeviceChunk.  Returns (chunks, rowCnt)."""
    chunks = [] if chunks is None else chunks
    n = chunk.NumRows()
    if n == 0:
        return chunks, rowCnt
    cols = (abi.Col * len(outputOffsets))(*[chunk.columns[o].col(n) for o in outputOffsets])
    cap = n * len(outputOffsets) * 11 + 16
    got = C.c_int64(0)
    if any(chunk.columns[o].tp == abi.BYTES for o in outputOffsets):  # string cells: the size of the response is asked first
        st = ctx.lib.tsq_rows_encode(ctx.h, cols, len(outputOffsets), None, n, None, 0, abi.COL_DEVICE, None, C.byref(got))
        if st not in (abi.OK, abi.ERR_INVALID):
            _lib.check(st, ctx.h)
        cap = got.value + 16
    dout = ctx.alloc(cap + 64)
    doffs = ctx.alloc((n + 1) * 8 + 64)
    try:
        got = C.c_int64(0)
        _lib.check(ctx.lib.tsq_rows_encode(ctx.h, cols, len(outputOffsets), None, n, C.c_void_p(dout), cap, abi.COL_DEVICE, C.c_void_p(doffs), C.byref(got)), ctx.h)
        raw = np.zeros(max(got.value, 1), np.uint8)
        offs = np.zeros(n + 1, np.int64)
        ctx.d2h(raw, dout)
        ctx.d2h(offs, doffs)
    finally:
        ctx.free(dout)
        ctx.free(doffs)
    lo = 0
    while lo < n:
        room = ROWS_PER_CHUNK - rowCnt % ROWS_PER_CHUNK  # rows the open piece still takes (64 when a new one starts)
        hi = min(n, lo + room)
        piece = bytes(raw[offs[lo]:offs[hi]])
        if rowCnt % ROWS_PER_CHUNK == 0:
            chunks.append(piece)
        else:
            chunks[-1] += piece
        rowCnt += hi - lo
        lo = hi
    return chunks, rowCnt


def fillUpChunkResponse(ctx, chunk, outputOffsets, chunks=None):
    """The column-major answer (upstream's tipb.EncodeType_TypeChunk; TinySQL ships the codec, util/chunk/codec.go:28-143, and answers
    with datum rows): every batch of the DAG's output becomes ONE wire chunk — chunk.Codec.Encode of the requested columns on the GPU
    (tsq_chunk_encode).  The SQL side reads it back with chunk.Decoder (tinysql_amd/chunk_codec.py): a copy instead of a parse."""
    chunks = [] if chunks is None else chunks
    n = chunk.NumRows()
    if n == 0:
        return chunks
    cols = (abi.Col * len(outputOffsets))(*[chunk.columns[o].col(n) for o in outputOffsets])
    need = C.c_int64(0)
    _lib.check(ctx.lib.tsq_chunk_encode(ctx.h, cols, len(outputOffsets), n, None, 0, abi.COL_DEVICE, C.byref(need)), ctx.h)
    dout = ctx.alloc(need.value + 64)
    try:
        _lib.check(ctx.lib.tsq_chunk_encode(ctx.h, cols, len(outputOffsets), n, C.c_void_p(dout), need.value, abi.COL_DEVICE, C.byref(need)), ctx.h)
        raw = np.zeros(need.value, np.uint8)
        ctx.d2h(raw, dout)
    finally:
        ctx.free(dout)
    chunks.append(raw.tobytes())
    return chunks


class SelectResponse:
    """tipb.SelectResponse as far as this path fills it: Chunks (RowsData byte strings), OutputCounts, Error."""

    def __init__(self):
        self.Chunks, self.OutputCounts, self.Error = [], None, None


def buildDAG(ctx, executors, pairs, store=None, kvRanges=None, startTS=None):
    """cop_handler_dag.go:149-160: chain the executors, each taking the previous one as its source.  executors: a list of
    ("TableScan", [ColInfo...]) | ("Selection", [conditions]) | ("Aggregation", aggFuncs, groupByCols) |
    ("TopN", orderByCols, desc, limit) | ("Limit", n); pairs = (keys, values, value_offsets) of the scanned ranges.
    With `store` (an mvcc.MvccStore) the scan reads kvRanges at startTS from it instead of `pairs`; ("TableScan", columns, desc) and
    ("IndexScan", types, colsLen, pkStatus, desc, unique) may then name the direction, and the index scan whether the index is unique
    (IndexScan.Unique: point-shaped ranges are read with Get only then)."""
    src = None
    for e in executors:
        tp = e[0]
        if tp == "TableScan" and store is not None:
            cur = tableScanExec.from_store(ctx, e[1], store, kvRanges, startTS, bool(e[2]) if len(e) > 2 else False)
        elif tp == "IndexScan" and store is not None:
            cur = indexScanExec.from_store(ctx, e[1], e[2], e[3], store, kvRanges, startTS, bool(e[4]) if len(e) > 4 else False,
                                           unique=bool(e[5]) if len(e) > 5 else False)
        elif tp == "TableScan":
            cur = tableScanExec(ctx, e[1], *pairs)
        elif tp == "Selection":
            cur = selectionExec(ctx, src, e[1])
        elif tp == "Aggregation":
            cur = hashAggExec(ctx, src, e[1], e[2])
        elif tp == "TopN":
            cur = topNExec(ctx, src, e[1], e[2], e[3])
        elif tp == "Limit":
            cur = limitExec(ctx, src, e[1])
        else:
            raise _lib.TsqError(abi.ERR_UNSUPPORTED, "this exec type %s doesn't support yet." % tp)  # cop_handler_dag.go:141-144
        src = cur
    return src


def handleCopDAGRequest(ctx, executors, outputOffsets, pairs, encodeType="default", store=None, kvRanges=None, startTS=None):
    """cop_handler_dag.go:49-83: run the DAG to its end, encode the rows, cut them into chunks.  An executor error becomes
    SelectResponse.Error (toPBError) and no chunks, like the reference.  encodeType "chunk": the response's Chunks are wire chunks
    (fillUpChunkResponse) instead of 64-row pieces of datum rows.  store / kvRanges / startTS in place of pairs: the scan reads the
    ranges from an mvcc.MvccStore; a lock it meets leaves the handler as mvcc.ErrLocked (the reference returns the lock error, not a
    response: cop_handler_dag.go:56-58) and no partial response is produced."""
    resp = SelectResponse()
    resp.EncodeType = encodeType
    e = buildDAG(ctx, executors, pairs, store, kvRanges, startTS)
    scan = e
    while scan.children:
        scan = scan.children[0]
    rows = 0
    try:
        e.Open()
        while True:
            chk = e.Next()
            if chk.NumRows() == 0:
                break
            if encodeType == "chunk":
                resp.Chunks = fillUpChunkResponse(ctx, chk, outputOffsets, resp.Chunks)
            else:
                resp.Chunks, rows = fillUpData4SelectResponse(ctx, chk, outputOffsets, resp.Chunks, rows)
        resp.OutputCounts = scan.Counts() if hasattr(scan, "Counts") else None
    except ErrLocked:
        raise
    except _lib.TsqError as err:
        resp.Chunks, resp.Error = [], err.message
    finally:
        e.Close()
    return resp


# ------------------------------------------------------------------------------------------------ handleCopAnalyzeRequest (analyze.go:34-219)
class AnalyzeColumnsResp:
    """tipb.AnalyzeColumnsResp: PkHist (statistics.Histogram of the handle column, or None) and one SampleCollector per other column."""

    def __init__(self, PkHist=None, Collectors=()):
        self.PkHist, self.Collectors = PkHist, list(Collectors)


class AnalyzeIndexResp:
    """tipb.AnalyzeIndexResp: Hist over the encoded index keys (bounds = the EncodeKey bytes of the index columns) and Cms over every
    prefix of 1 .. NumColumns columns."""

    def __init__(self, Hist=None, Cms=None):
        self.Hist, self.Cms = Hist, Cms


def handleAnalyzeColumnsReq(ctx, columns, pairs, BucketSize, SampleSize, SketchSize, CmsketchDepth=0, CmsketchWidth=0, seed=0, batch_rows=1 << 22):
    """analyze.go:123-219: scan the ranges' rows; the first column may be the PK handle, its values go to a SortedBuilder (the scan returns
    them in handle order); every other column goes to the collector as the datum the scan hands on (EncodeValue form), the FM sketch over
    the bytes datum of it (analyzeColumnsExec.getNext, :226-243).  columns: rowcodec.ColInfo list; pairs: (keys, values, value_offsets)."""
    from .statistics import AnalyzeCollector, SortedBuilder
    scan = tableScanExec(ctx, columns, *pairs, batch_rows=batch_rows)
    first = 1 if columns and columns[0].IsPKHandle else 0
    types = scan.Schema()
    pk = SortedBuilder(ctx, types[0], BucketSize) if first else None
    col = None
    if len(types) > first:
        col = AnalyzeCollector(ctx, types[first:], SampleSize, SketchSize, CmsketchDepth, CmsketchWidth, wrap_bytes=True, seed=seed)
    try:
        scan.Open()
        while True:
            chk = scan.Next()
            n = chk.NumRows()
            if n == 0:
                break
            if pk:
                pk.push(chk.columns[0], n)
            if col:
                col.push(DeviceChunk(chk.columns[first:], n))
        return AnalyzeColumnsResp(pk.Hist() if pk else None, col.finish() if col else [])
    finally:
        scan.Close()
        for h in (pk, col):
            if h:
                h.close()


def _encode_key_prefix(ctx, chunk, k):
    """EncodeKey of the first k columns of every row, concatenated per row -> a var-len device column (data, offsets) + its bytes"""
    n = chunk.NumRows()
    cols = (abi.Col * k)(*[chunk.columns[i].col(n) for i in range(k)])
    flags = (C.c_uint32 * k)(*([abi.ENC_COMPARABLE] * k))
    got = C.c_int64(0)
    st = ctx.lib.tsq_rows_encode(ctx.h, cols, k, flags, n, None, 0, abi.COL_DEVICE, None, C.byref(got))  # (asks for the size)
    if st not in (abi.OK, abi.ERR_INVALID):
        _lib.check(st, ctx.h)
    out = DeviceColumn(ctx, abi.BYTES, n, with_bitmap=False, cap_bytes=got.value + 16)
    try:
        _lib.check(ctx.lib.tsq_rows_encode(ctx.h, cols, k, flags, n, C.c_void_p(out.data), got.value + 16, abi.COL_DEVICE, C.c_void_p(out.offsets), C.byref(got)), ctx.h)
    except Exception:
        out.free()
        raise
    return out


def handleAnalyzeIndexReq(ctx, types, NumColumns, keys, key_offsets, BucketSize, CmsketchDepth=0, CmsketchWidth=0, batch_rows=1 << 22):
    """analyze.go:63-116: scan the index range; per pair the encoded values of its first 1 .. NumColumns columns, concatenated, feed ONE CM
    sketch (:94-100) and the full key a SortedBuilder (:101).  types: the index columns' types; keys / key_offsets: the index keys."""
    from .statistics import AnalyzeCollector, CMSketch, SortedBuilder
    m = int(NumColumns)
    scan = indexScanExec(ctx, list(types)[:m], m, indexScanExec.PrimaryKeyNotExists, keys, key_offsets, batch_rows=batch_rows)
    hist = SortedBuilder(ctx, abi.BYTES, BucketSize)
    cms = AnalyzeCollector(ctx, [abi.BYTES] * m, 0, 1, CmsketchDepth, CmsketchWidth, col_flags=[abi.AN_RAW] * m) if CmsketchDepth else None
    try:
        scan.Open()
        while True:
            chk = scan.Next()
            n = chk.NumRows()
            if n == 0:
                break
            prefixes = []
            try:
                for k in range(1 if cms else m, m + 1):
                    prefixes.append(_encode_key_prefix(ctx, chk, k))
                hist.push(prefixes[-1], n)
                if cms:
                    cms.push(DeviceChunk(prefixes, n))
            finally:
                for p in prefixes:
                    p.free()
        cm = None
        if cms:
            cm = CMSketch(CmsketchDepth, CmsketchWidth)
            for c in cms.finish():
                cm.MergeCMSketch(c.CMSketch)
        return AnalyzeIndexResp(hist.Hist(), cm)
    finally:
        scan.Close()
        hist.close()
        if cms:
            cms.close()
