"""The duplicate-key checker over libtsq (tsq_dupcheck_*, tsq_rows_equal; include/tsq.h "Duplicate keys"): what InsertExec and
ReplaceExec ask the store row by row (table/tables/tables.go:528-581, executor/replace.go:53-196), settled for a whole statement in HBM.
Everything below is plumbing around the C-ABI; every array a method takes or returns is a device pointer unless it says otherwise."""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib


class KeyExistsError(_lib.TsqError):
    """kv.ErrKeyExists: `row` (of the statement) met an entry with its key in `stream`; dup_handle = the handle that entry points to —
    the stored row's, or the handle of the FIRST statement row with that key (from_store = False, dup_row = that row)"""

    def __init__(self, row, stream, dup_handle, from_store=True, dup_row=-1):
        _lib.TsqError.__init__(self, abi.ERR_KEY_EXISTS, "duplicate entry: statement row %d, stream %d, handle %d" % (row, stream, dup_handle))
        self.row, self.stream, self.dup_handle, self.from_store, self.dup_row = row, stream, dup_handle, from_store, dup_row


class HandleStream:
    """the PK handle as a unique key: the table's handles (device, ascending)"""

    def __init__(self, handles, n):
        self.handles, self.n = handles, n


class IndexStream:
    """a unique index: the store's distinct entries in key order (device): keys, key_offsets (n + 1), handles; float_key: a FLOAT /
    DOUBLE column is part of the index"""

    def __init__(self, keys, key_offsets, key_bytes, handles, n, float_key=False):
        self.keys, self.key_offsets, self.key_bytes, self.handles, self.n, self.float_key = keys, key_offsets, key_bytes, handles, n, float_key


class DupChecker:
    def __init__(self, ctx, streams, mode, table_handles=None, n_table_rows=0):
        self.ctx, self.lib, self.mode, self.n_streams = ctx, ctx.lib, mode, len(streams)
        self.kinds = [abi.DUP_HANDLE if isinstance(s, HandleStream) else abi.DUP_INDEX for s in streams]
        arr = (abi.DupStream * max(len(streams), 1))()
        for a, s, k in zip(arr, streams, self.kinds):
            a.kind, a.handles, a.n = k, s.handles, s.n
            if k == abi.DUP_INDEX:
                a.keys, a.key_offsets, a.key_bytes, a.flags = s.keys, s.key_offsets, s.key_bytes, abi.DUP_FLOAT_KEY if s.float_key else 0
        h = C.c_void_p()
        self.h = None
        _lib.check(self.lib.tsq_dupcheck_create(ctx.h, arr, len(streams), mode, C.c_void_p(table_handles) if table_handles else None, n_table_rows,
                                                C.byref(h)), ctx.h)
        self.h = h
        self.rows = 0

    def push(self, keys, n):
        """keys: per stream a device pointer to n handles (HANDLE stream) or (keys, key_offsets, key_bytes, distinct or None)"""
        arr = (abi.DupKeys * max(self.n_streams, 1))()
        assert len(keys) == self.n_streams
        for a, k, kind in zip(arr, keys, self.kinds):
            if kind == abi.DUP_HANDLE:
                a.handles = k
            else:
                a.keys, a.key_offsets, a.key_bytes, a.distinct = k
        _lib.check(self.lib.tsq_dupcheck_push(self.h, arr, self.n_streams, n), self.h)
        self.rows += n

    def match_insert(self):
        """INSERT mode: None, or the statement's KeyExistsError (not raised: the caller knows the handles of its own rows)"""
        cf = abi.DupConflict()
        st = self.lib.tsq_dupcheck_match(self.h, C.byref(cf), None, None, None, None, None)
        if st == abi.ERR_KEY_EXISTS:
            return KeyExistsError(cf.row, cf.stream, cf.dup_handle, bool(cf.from_store), cf.dup_row)
        _lib.check(st, self.h)
        return None

    def match_replace(self, cand_row, cand_handle, cand_ord):
        """REPLACE mode: fills the three device arrays (rows int64 each) -> (rows with a statement-row candidate, with a stored one)"""
        nb, ns = C.c_int64(0), C.c_int64(0)
        _lib.check(self.lib.tsq_dupcheck_match(self.h, None, C.c_void_p(cand_row), C.c_void_p(cand_handle), C.c_void_p(cand_ord), C.byref(nb), C.byref(ns)),
                   self.h)
        return nb.value, ns.value

    def resolve(self, equal_flags, rowid_base, added, put, handles_out, removed_handles, removed_ords, cap_removed):
        """-> abi.DupResult.  On "buffers too small" the TsqError carries .needed = the pairs needed"""
        res = abi.DupResult()
        st = self.lib.tsq_dupcheck_resolve(self.h, C.c_void_p(equal_flags), rowid_base, C.c_void_p(added), C.c_void_p(put),
                                           C.c_void_p(handles_out) if handles_out else None, C.c_void_p(removed_handles) if removed_handles else None,
                                           C.c_void_p(removed_ords) if removed_ords else None, cap_removed, C.byref(res))
        if st != abi.OK:
            e = _lib.TsqError(st, _lib.last_error(self.h))
            e.needed = res.n_removed_store
            raise e
        return res

    def stats(self):
        a, b, c, d, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_dupcheck_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(ms)), self.h)
        return {"rows": a.value, "pushes": b.value, "cand_batch": c.value, "cand_store": d.value, "kernel_ms": ms.value}

    def reset(self):
        """the next statement against the same store"""
        _lib.check(self.lib.tsq_dupcheck_reset(self.h), self.h)
        self.rows = 0

    def cancel(self):
        _lib.check(self.lib.tsq_dupcheck_cancel(self.h), self.h)

    def close(self):
        if self.h:
            self.lib.tsq_dupcheck_destroy(self.h)
            self.h = None


def rows_equal(ctx, cols_a, idx_a, cols_b, idx_b, n, flags_out):
    """tsq_rows_equal: cols_a / cols_b = lists of abi.Col (device columns), idx_a / idx_b = device int64 arrays or None (pair i takes
    row i), flags_out = device bytes"""
    assert len(cols_a) == len(cols_b)
    nc = len(cols_a)
    ca, cb = (abi.Col * max(nc, 1))(*cols_a), (abi.Col * max(nc, 1))(*cols_b)
    _lib.check(ctx.lib.tsq_rows_equal(ctx.h, ca, C.c_void_p(idx_a) if idx_a else None, cb, C.c_void_p(idx_b) if idx_b else None, nc, n,
                                      C.c_void_p(flags_out)), ctx.h)


class DevArray:
    """a numpy array's bytes in HBM (a small helper for the callers of this module: uploads, read-backs)"""

    def __init__(self, ctx, host=None, nbytes=0):
        self.ctx = ctx
        if host is not None:
            host = np.ascontiguousarray(host)
            nbytes = host.nbytes
        self.nbytes = nbytes
        self.p = ctx.alloc(max(nbytes, 1) + 64)
        if host is not None and nbytes:
            ctx.h2d(self.p, host)

    def read(self, dtype, count):
        out = np.zeros(max(count, 1), dtype=dtype)
        if count:
            self.ctx.d2h(out, self.p)
        return out[:count]

    def free(self):
        if self.p:
            self.ctx.free(self.p)
        self.p = None
