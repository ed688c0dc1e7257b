"""Mirror of the ADD INDEX backfill worker for the harness (ddl/index.go:742-921): the rows of one handle range -> the KV pairs of the new
index, computed on the GPU by libtsq.

The reference's backfillIndexInTxn runs, per transaction of 128 rows: fetchRowColVals (scan the range, decode the index columns of
every row) -> checkUniqueKey (GenIndexKey per row, look the keys up in the store, and catch duplicates INSIDE the batch, :849-853) ->
index.Create per row.  Here a batch is a device chunk of `batch_rows` rows (as many as fit HBM: a batch is one launch, not one row loop):
    fetchRowColVals            = coprocessor.tableScanExec (tsq_rowkeys_decode + tsq_rowcodec_decode), the index columns picked by pointer
    GenIndexKey + Create's value = tablecodec.GenIndexKeys (tsq_indexkeys_encode)
    checkUniqueKey, in-batch half = the distinct rows compacted (tsq_chunk_compact) and grouped by the index columns
                                 (tsq_agg_create_keys + tsq_agg_num_groups): fewer groups than distinct rows = two rows with equal
                                 non-NULL values = kv.ErrKeyExists
What stays with the host KV store: the look-up of keys that already exist in the store (the other half of checkUniqueKey, :820-847),
the row locks (txn.LockKeys) and the transaction itself — the caller writes the returned pairs through its own txn.
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib
from . import tablecodec
from .gpu_pipeline import DeviceChunk, DeviceColumn

# kv.ErrKeyExists (kv/error.go:41-42): terror.ClassKV, mysql.ErrDupEntry, returned unformatted by checkUniqueKey (ddl/index.go:844)
ErrKeyExists = "[kv:1062]Duplicate entry '%-.192s' for key %d"


class addIndexTaskContext:
    """ddl/index.go:553-559 + the pairs the transaction would have written"""

    def __init__(self):
        self.scanCount = self.addedCount = 0
        self.keys, self.key_offsets = np.zeros(0, np.uint8), np.zeros(1, np.int64)
        self.values, self.value_offsets = np.zeros(0, np.uint8), np.zeros(1, np.int64)

    def _append(self, keys, ko, vals, vo):
        self.key_offsets = np.concatenate([self.key_offsets, ko[1:] + self.keys.size])
        self.value_offsets = np.concatenate([self.value_offsets, vo[1:] + self.values.size])
        self.keys, self.values = np.concatenate([self.keys, keys]), np.concatenate([self.values, vals])

    def pairs(self):
        """[(key bytes, value bytes)] in scan order"""
        k, v = self.keys.tobytes(), self.values.tobytes()
        return [(k[self.key_offsets[i]:self.key_offsets[i + 1]], v[self.value_offsets[i]:self.value_offsets[i + 1]]) for i in range(len(self.key_offsets) - 1)]


class addIndexWorker:
    """ddl.addIndexWorker (ddl/index.go:527-551)."""

    def _check_unique_in_batch(self, ctx, cols, n, distinct):
        """rows of the batch with equal non-NULL index values: the in-batch half of checkUniqueKey (ddl/index.go:849-853)"""
        lib = ctx.lib
        types = [c.tp for c in cols]
        src = DeviceChunk(cols, n)
        out = [DeviceColumn(ctx, t, n, cap_bytes=c.nbytes(n) if t == abi.BYTES else 0) for t, c in zip(types, cols)]
        h = C.c_void_p()
        try:
            oc = (abi.Col * len(out))(*[c.col(n) for c in out])
            m = C.c_int64(0)
            _lib.check(lib.tsq_chunk_compact(ctx.h, src.cols(), len(cols), n, C.c_void_p(distinct), oc, C.byref(m)), ctx.h)
            if m.value < 2:
                return
            cfg = abi.AggCfg()
            cfg.n_group_keys, cfg.n_aggs = 0, 1
            cfg.aggs[0].func, cfg.aggs[0].mode, cfg.aggs[0].arg_type = abi.AGG_COUNT, abi.MODE_COMPLETE, abi.I64
            cfg.aggs[0].arg_col = cfg.aggs[0].arg_col2 = -1  # COUNT(*)
            cfg.n_input_cols = len(types)
            for i, t in enumerate(types):
                cfg.input_types[i] = t
            cfg.est_groups, cfg.max_chunk_size = m.value, 1024
            kc, kt = (C.c_int32 * len(types))(*range(len(types))), (C.c_int32 * len(types))(*types)
            _lib.check(lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), kc, kt, len(types), C.byref(h)), ctx.h)
            dc = (abi.Col * len(out))(*[c.col(m.value) for c in out])
            _lib.check(lib.tsq_agg_push(h, dc, len(out), m.value), h)
            _lib.check(lib.tsq_agg_finish(h), h)
            ng = C.c_int64(0)
            _lib.check(lib.tsq_agg_num_groups(h, C.byref(ng)), h)
            if ng.value < m.value:
                raise _lib.TsqError(abi.ERR_INVALID, ErrKeyExists)
        finally:
            if h:
                lib.tsq_agg_destroy(h)
            for c in out:
                c.free()

    def backfill(self, ctx, scan_executor, index_cols, tableID, indexID, unique, batch_rows=1 << 22):
        """backfillIndexInTxn (ddl/index.go:865-921) for the handle range `scan_executor` (a coprocessor.tableScanExec, not yet open) covers:
        index_cols = the positions of the index columns in the scan's schema, in index order.  Returns an addIndexTaskContext with the KV
        pairs of the range in scan order and scanCount / addedCount; two rows of one batch with equal non-NULL values of a unique index raise
        TsqError(kv.ErrKeyExists).  Keys that already exist in the store, the row locks and the transaction are the caller's (see the
        module text): addedCount counts every scanned row, none is skipped here."""
        task = addIndexTaskContext()
        scan_executor.batch = (max(int(batch_rows), 1) + 7) & ~7
        scan_executor.Open()
        try:
            while True:
                lo = scan_executor.pos
                chk = scan_executor.Next()
                n = chk.NumRows()
                if n == 0:
                    break
                cols = [chk.columns[i] for i in index_cols]
                kvs = tablecodec.GenIndexKeys(ctx, tableID, indexID, unique, DeviceChunk(cols, n), scan_executor.dh + 8 * lo)
                try:
                    if unique:
                        self._check_unique_in_batch(ctx, cols, n, kvs.distinct)
                    keys, ko, vals, vo, _ = kvs.to_host()
                finally:
                    kvs.free()
                task._append(keys, ko, vals, vo)
                task.scanCount += n
                task.addedCount += n
        finally:
            scan_executor.Close()
        return task
