"""The transaction's write buffer in HBM: kv.memDbBuffer (kv/memdb_buffer.go) as the two-phase committer walks it
(store/tikv/2pc.go:115-172), over tsq_membuf_* (include/tsq.h "Transaction buffer").  Pushes are copied; finish() sorts them, keeps
the last write of every key and leaves a device-resident, strictly ascending tsq_mvcc_write_req that tsq_mvcc_prewrite / commit /
rollback take as it is (mvcc.write_membuffer)."""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib
from .dupcheck import DevArray
from .mvcc import ErrLocked, Pairs


class ErrNotExist(KeyError):
    """kv.ErrNotExist: memDbBuffer.Get of a key the buffer does not hold"""


class MemBuffer:
    """tsq_membuf.  set_packed / delete_packed / lock_packed push device or host arrays at once; Set / Delete / LockKeys collect single
    entries on the host and push them, in order, before the next packed push or finish()."""

    def __init__(self, ctx, entry_size_limit=0, total_size_limit=0):
        self.ctx, self.lib, self.h = ctx, ctx.lib, None
        cfg = abi.MembufCfg(entry_size_limit, total_size_limit, 0, 0)
        h = C.c_void_p()
        _lib.check(self.lib.tsq_membuf_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
        self.h = h
        self._pending = []   # [(kind, key, value)] of the host conveniences
        self.result = None   # the dict of the last finish()

    # ------------------------------------------------------------------ packed pushes
    @staticmethod
    def _ptr(a):
        """a numpy array (host) or an int / None (a device pointer)"""
        if isinstance(a, np.ndarray):
            return a.ctypes.data if a.size else None
        return a

    def push_packed(self, kind, keys, key_offsets, key_bytes, n, values=None, value_offsets=None, value_bytes=0, device=False):
        """one tsq_membuf_push.  keys / values / offsets: numpy arrays (host), or with device=True device pointers; key_offsets None = keys
        of key_bytes / n bytes each.  Raises TsqError with .error_row on a refused row; the push then added nothing."""
        self._flush()
        self._push(kind, keys, key_offsets, key_bytes, n, values, value_offsets, value_bytes, device)

    def _push(self, kind, keys, key_offsets, key_bytes, n, values, value_offsets, value_bytes, device):
        row = C.c_int64(-1)
        st = self.lib.tsq_membuf_push(self.h, kind, C.c_void_p(self._ptr(keys)), C.c_void_p(self._ptr(key_offsets)), key_bytes, n, C.c_void_p(self._ptr(values)),
                                      C.c_void_p(self._ptr(value_offsets)), value_bytes, abi.COL_DEVICE if device else 0, C.byref(row))
        if st != abi.OK:
            e = _lib.TsqError(st, _lib.last_error(self.h))
            e.error_row = row.value
            raise e
        self.result = None

    def set_packed(self, keys, key_offsets, key_bytes, n, values, value_offsets, value_bytes, device=False):
        self.push_packed(abi.MEMBUF_SET, keys, key_offsets, key_bytes, n, values, value_offsets, value_bytes, device)

    def delete_packed(self, keys, key_offsets, key_bytes, n, device=False):
        self.push_packed(abi.MEMBUF_DELETE, keys, key_offsets, key_bytes, n, device=device)

    def lock_packed(self, keys, key_offsets, key_bytes, n, device=False):
        self.push_packed(abi.MEMBUF_LOCK, keys, key_offsets, key_bytes, n, device=device)

    # ------------------------------------------------------------------ host conveniences
    def Set(self, k, v):
        self._pending.append((abi.MEMBUF_SET, bytes(k), bytes(v)))

    def Delete(self, k):
        self._pending.append((abi.MEMBUF_DELETE, bytes(k), b""))

    def LockKeys(self, *keys):
        self._pending += [(abi.MEMBUF_LOCK, bytes(k), b"") for k in keys]

    @staticmethod
    def _pack(cells):
        offs = np.zeros(len(cells) + 1, dtype=np.int64)
        if cells:
            offs[1:] = np.cumsum([len(c) for c in cells])
        return np.frombuffer(b"".join(cells), dtype=np.uint8).copy(), offs

    def _flush(self):
        """the pending single entries as one push per run of equal kind, in order.  A refused run raises (error_row counts among the
        pending entries); the runs in front of it are in, the refused run is dropped whole — a refused push adds nothing — and the
        entries behind it stay pending."""
        pend, self._pending = self._pending, []
        at = 0
        while at < len(pend):
            end = at
            while end < len(pend) and pend[end][0] == pend[at][0]:
                end += 1
            kb, ko = self._pack([p[1] for p in pend[at:end]])
            vb, vo = self._pack([p[2] for p in pend[at:end]])
            try:
                self._push(pend[at][0], kb, ko, kb.size, end - at, vb, vo, vb.size, False)
            except _lib.TsqError as e:
                e.error_row += at if e.error_row >= 0 else 0  # (the row among the pending entries)
                self._pending = pend[end:] + self._pending
                raise
            at = end

    # ------------------------------------------------------------------ finish and what follows it
    def finish(self):
        """tsq_membuf_finish -> dict(n_entries, puts, dels, locks, size, primary_index, sort_passes, kernel_ms)"""
        self._flush()
        res = abi.MembufResult()
        _lib.check(self.lib.tsq_membuf_finish(self.h, C.byref(res)), self.h)
        self.result = {k: getattr(res, k) for k, _ in abi.MembufResult._fields_}
        return self.result

    def _finished(self):
        if self.result is None or self._pending:
            self.finish()
        return self.result

    def request(self):
        """the buffer's own device arrays as an abi.MvccWriteReq (primary and timestamps left to the caller); valid until the next push"""
        self._finished()
        req = abi.MvccWriteReq()
        _lib.check(self.lib.tsq_membuf_request(self.h, C.byref(req)), self.h)
        return req

    def get_packed(self, keys, key_offsets, key_bytes, n, device=False):
        """batched Get -> int64 [n]: the entry index of every key, -1 = ErrNotExist"""
        self._finished()
        out = np.full(max(n, 1), -1, dtype=np.int64)
        _lib.check(self.lib.tsq_membuf_get(self.h, C.c_void_p(self._ptr(keys)), C.c_void_p(self._ptr(key_offsets)), key_bytes, n,
                                           abi.COL_DEVICE if device else 0, out.ctypes.data), self.h)
        return out[:n]

    def Get(self, keys):
        """memDbBuffer.Get of one key or a list of keys: the value (b"" for a deleted key); raises ErrNotExist — for a lock-only key
        too.  Reads back two value offsets and the value bytes per hit, nothing else of the buffer."""
        single = isinstance(keys, (bytes, bytearray))
        ks = [bytes(keys)] if single else [bytes(k) for k in keys]
        kb, ko = self._pack(ks)
        idx = self.get_packed(kb, ko, kb.size, len(ks))
        req = self.request()
        out = []
        for k, i in zip(ks, idx):
            if i < 0:
                raise ErrNotExist(k)
            vo = np.zeros(2, dtype=np.int64)
            self.ctx.d2h(vo, req.value_offsets + 8 * int(i))
            v = np.zeros(max(int(vo[1] - vo[0]), 1), dtype=np.uint8)
            if vo[1] > vo[0]:
                self.ctx.d2h(v[:int(vo[1] - vo[0])], req.values + int(vo[0]))
            out.append(v[:int(vo[1] - vo[0])].tobytes())
        return out[0] if single else out

    def entries(self):
        """[(op, key, value)] of the finished buffer, read back — for tests and small transactions"""
        req = self.request()
        n = req.n_keys
        ko, vo = np.zeros(n + 1, dtype=np.int64), np.zeros(n + 1, dtype=np.int64)
        ops, kb, vb = np.zeros(max(n, 1), dtype=np.uint8), np.zeros(max(req.key_bytes, 1), dtype=np.uint8), np.zeros(max(req.value_bytes, 1), dtype=np.uint8)
        self.ctx.d2h(ko, req.key_offsets)
        self.ctx.d2h(vo, req.value_offsets)
        if n:
            self.ctx.d2h(ops[:n], req.ops)
        if req.key_bytes:
            self.ctx.d2h(kb[:req.key_bytes], req.keys)
        if req.value_bytes:
            self.ctx.d2h(vb[:req.value_bytes], req.values)
        kb, vb = kb.tobytes(), vb.tobytes()
        return [(int(ops[i]), kb[ko[i]:ko[i + 1]], vb[vo[i]:vo[i + 1]]) for i in range(n)]

    # ------------------------------------------------------------------ the mem readers' view (tsq_membuf_scan / _points / _fetch / _dirty)
    def _fetch(self, res, counts=None):
        """the pairs of the last scan in fresh device buffers -> mvcc.Pairs (the form tsq_mvcc_fetch writes); .scan holds the scan's counts"""
        p = Pairs(self.ctx, res.n_pairs, res.key_bytes, res.value_bytes, counts, res.positions)
        p.scan = {k: getattr(res, k) for k, _ in abi.MembufScanResult._fields_}
        try:
            _lib.check(self.lib.tsq_membuf_fetch(self.h, C.c_void_p(p.keys.p), res.key_bytes, C.c_void_p(p.key_offsets.p), C.c_void_p(p.values.p), res.value_bytes,
                                                 C.c_void_p(p.value_offsets.p)), self.h)
        except Exception:
            p.free()
            raise
        return p

    def scan_packed(self, range_bytes, range_offsets, n_ranges, desc=False, device=False, want_counts=False):
        """one tsq_membuf_scan + tsq_membuf_fetch.  range_bytes / range_offsets: numpy arrays (host), or with device=True device
        pointers, laid out as tsq_mvcc_scan's.  -> mvcc.Pairs (.counts = the pairs of every range when want_counts)"""
        self._finished()
        res = abi.MembufScanResult()
        counts = np.zeros(max(n_ranges, 1), dtype=np.int64) if want_counts else None
        _lib.check(self.lib.tsq_membuf_scan(self.h, C.c_void_p(self._ptr(range_bytes)), C.c_void_p(self._ptr(range_offsets)), n_ranges,
                                            abi.COL_DEVICE if device else 0, 1 if desc else 0, C.byref(res), C.c_void_p(counts.ctypes.data if want_counts else None)),
                   self.h)
        return self._fetch(res, counts[:n_ranges].tolist() if want_counts else None)

    def scan(self, ranges, desc=False, want_counts=False):
        """iterTxnMemBuffer over [(start, end)] byte ranges (b"" start: from the first key; b"" end: to the last): the buffer's PUT pairs
        inside every range, in the order of the ranges, the whole sequence reversed for desc -> mvcc.Pairs in HBM"""
        cells = [bytes(b) for r in ranges for b in r]
        rb, ro = self._pack(cells)
        return self.scan_packed(rb, ro, len(ranges), desc, False, want_counts)

    def scan_points_packed(self, keys, key_offsets, key_bytes, n, device=False):
        """one tsq_membuf_scan_points + fetch: keys as in a push (key_offsets None: fixed length) -> mvcc.Pairs, input order kept"""
        self._finished()
        res = abi.MembufScanResult()
        _lib.check(self.lib.tsq_membuf_scan_points(self.h, C.c_void_p(self._ptr(keys)), C.c_void_p(self._ptr(key_offsets)), key_bytes, n,
                                                   abi.COL_DEVICE if device else 0, C.byref(res)), self.h)
        return self._fetch(res)

    def scan_points(self, keys):
        kb, ko = self._pack([bytes(k) for k in keys])
        return self.scan_points_packed(kb, ko, kb.size, len(keys))

    def dirty_handles(self, table_id):
        """the table's dirty handles out of the buffer -> (added, n_added, deleted, n_deleted): two device int64 arrays (ctx.free them),
        each ascending; a handle deleted and re-inserted is in `added` only (include/tsq.h: the pinned departure)"""
        self._finished()
        na, nd = C.c_int64(0), C.c_int64(0)
        _lib.check(self.lib.tsq_membuf_dirty(self.h, table_id, C.byref(na), C.byref(nd)), self.h)
        added, deleted = self.ctx.alloc(max(na.value, 1) * 8 + 64), self.ctx.alloc(max(nd.value, 1) * 8 + 64)
        try:
            _lib.check(self.lib.tsq_membuf_dirty_fetch(self.h, C.c_void_p(added), C.c_void_p(deleted)), self.h)
        except Exception:
            self.ctx.free(added)
            self.ctx.free(deleted)
            raise
        return added, na.value, deleted, nd.value

    def Iter(self, start=b"", end=b""):
        """memDbBuffer.Iter(start, end) as iterTxnMemBuffer reads it: [(key, value)] of the PUT entries in [start, end), read back — for
        tests"""
        p = self.scan([(start, end)])
        try:
            return p.to_host()
        finally:
            p.free()

    def Len(self):
        return self._finished()["n_entries"]

    def Size(self):
        return self._finished()["size"]

    def close(self):
        if self.h:
            self.lib.tsq_membuf_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class UnionStore:
    """tsq_unionstore: a transaction's reads over its write buffer and its snapshot — BufferStore.Get and BufferStore.Iter /
    IterReverse with kv.UnionIter (kv/buffer_store.go:61-99, kv/union_iter.go:64-152).  `store` is an mvcc.MvccStore read at
    start_ts, `membuf` a MemBuffer or None (lazyMemBuffer never written); both are borrowed and must outlive this object.  The
    buffer is finished before every read, so a read sees every write made through `membuf` before it."""

    def __init__(self, ctx, store, membuf, start_ts):
        self.ctx, self.lib, self.h, self.store, self.membuf, self.start_ts = ctx, ctx.lib, None, store, membuf, start_ts
        h = C.c_void_p()
        if membuf is not None:
            membuf._finished()
        _lib.check(self.lib.tsq_unionstore_create(ctx.h, store.h, membuf.h if membuf is not None else None, C.c_uint64(start_ts), C.byref(h)), ctx.h)
        self.h = h

    def _locked(self):
        kl, pl, ts, ttl, op = C.c_int64(0), C.c_int64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        self.lib.tsq_unionstore_locked(self.h, None, 0, C.byref(kl), None, 0, C.byref(pl), C.byref(ts), C.byref(ttl), C.byref(op))  # (the lengths)
        key, prim = np.zeros(max(kl.value, 1), dtype=np.uint8), np.zeros(max(pl.value, 1), dtype=np.uint8)
        _lib.check(self.lib.tsq_unionstore_locked(self.h, key.ctypes.data, kl.value, C.byref(kl), prim.ctypes.data, pl.value, C.byref(pl), C.byref(ts), C.byref(ttl),
                                                  C.byref(op)), self.h)
        return ErrLocked(key[:kl.value].tobytes(), prim[:pl.value].tobytes(), ts.value, ttl.value, op.value)

    def _check(self, st, res):
        if st == abi.ERR_LOCKED:
            e = self._locked()
            e.n_pairs = res.n_pairs
            raise e
        _lib.check(st, self.h)

    def _fetch(self, res, counts=None):
        """the pairs of the last read in fresh device buffers -> mvcc.Pairs with .from_buffer (a device byte per pair: curIsDirty) and
        .scan (the read's counts)"""
        p = Pairs(self.ctx, res.n_pairs, res.key_bytes, res.value_bytes, counts, res.positions_snapshot + res.positions_buffer)
        p.scan = {k: getattr(res, k) for k, _ in abi.UnionStoreResult._fields_}
        p.from_buffer = DevArray(self.ctx, nbytes=res.n_pairs + 8)
        free = p.free

        def free_all():
            free()
            p.from_buffer.free()
        p.free = free_all
        try:
            _lib.check(self.lib.tsq_unionstore_fetch(self.h, C.c_void_p(p.keys.p), res.key_bytes, C.c_void_p(p.key_offsets.p), C.c_void_p(p.values.p), res.value_bytes,
                                                     C.c_void_p(p.value_offsets.p), C.c_void_p(p.from_buffer.p)), self.h)
        except Exception:
            p.free()
            raise
        return p

    def _ready(self):
        if self.membuf is not None:
            self.membuf._finished()

    def scan_packed(self, range_bytes, range_offsets, n_ranges, desc=False, limit=-1, device=False, want_counts=False, fetch=True):
        """one tsq_unionstore_scan (+ fetch): ranges laid out as tsq_mvcc_scan's, numpy arrays (host) or with device=True device pointers
        -> mvcc.Pairs; fetch=False -> the abi.UnionStoreResult alone.  Raises mvcc.ErrLocked (with .n_pairs)"""
        self._ready()
        res = abi.UnionStoreResult()
        counts = np.zeros(max(n_ranges, 1), dtype=np.int64) if want_counts else None
        ptr = MemBuffer._ptr
        st = self.lib.tsq_unionstore_scan(self.h, C.c_void_p(ptr(range_bytes)), C.c_void_p(ptr(range_offsets)), n_ranges, abi.COL_DEVICE if device else 0,
                                          1 if desc else 0, -1 if limit is None else limit, C.byref(res), C.c_void_p(counts.ctypes.data if want_counts else None))
        self._check(st, res)
        if not fetch:
            return res
        return self._fetch(res, counts[:n_ranges].tolist() if want_counts else None)

    def scan(self, ranges, desc=False, limit=-1, want_counts=False):
        """the merged pairs of [(start, end)] byte ranges, range by range in the order given, every range descending with desc"""
        rb, ro = MemBuffer._pack([bytes(b) for r in ranges for b in r])
        return self.scan_packed(rb, ro, len(ranges), desc, limit, False, want_counts)

    def get_packed(self, keys, key_offsets, key_bytes, n, device=False, fetch=True):
        """one tsq_unionstore_get (+ fetch): keys as in a push (key_offsets None: fixed length) -> (found uint8 [n], mvcc.Pairs of the found
        keys in input order, or the result alone)"""
        self._ready()
        res = abi.UnionStoreResult()
        found = np.zeros(max(n, 1), dtype=np.uint8)
        ptr = MemBuffer._ptr
        st = self.lib.tsq_unionstore_get(self.h, C.c_void_p(ptr(keys)), C.c_void_p(ptr(key_offsets)), key_bytes, n, abi.COL_DEVICE if device else 0,
                                         C.byref(res), C.c_void_p(found.ctypes.data))
        self._check(st, res)
        return found[:n], (self._fetch(res) if fetch else res)

    def scan_points(self, keys):
        """the pairs of the keys the union store holds, input order kept -> mvcc.Pairs (.found: one flag per key)"""
        kb, ko = MemBuffer._pack([bytes(k) for k in keys])
        found, p = self.get_packed(kb, ko, kb.size, len(keys))
        p.found = found
        return p

    def Get(self, keys):
        """BufferStore.Get of one key or a list of keys: the value, or None for ErrNotExist; raises mvcc.ErrLocked"""
        single = isinstance(keys, (bytes, bytearray))
        ks = [bytes(keys)] if single else [bytes(k) for k in keys]
        p = self.scan_points(ks)
        try:
            vals = iter([v for _, v in p.to_host()])
        finally:
            p.free()
        out = [next(vals) if f else None for f in p.found]
        return out[0] if single else out

    def Iter(self, start=b"", end=b""):
        """BufferStore.Iter(start, end): a host generator of (key, value) — for tests"""
        p = self.scan([(start, end)])
        try:
            pairs = p.to_host()
        finally:
            p.free()
        yield from pairs

    def IterReverse(self, k=b""):
        """BufferStore.IterReverse(k): the pairs below k, descending — for tests"""
        p = self.scan([(b"", k)], desc=True)
        try:
            pairs = p.to_host()
        finally:
            p.free()
        yield from pairs

    def stats(self):
        a = [C.c_int64(0) for _ in range(5)]
        route, ms = C.c_int32(0), C.c_double(0)
        _lib.check(self.lib.tsq_unionstore_stats(self.h, *[C.byref(x) for x in a], C.byref(route), C.byref(ms)), self.h)
        return dict(zip(("scans", "merged", "snapshot_only", "gets", "pairs"), [x.value for x in a]), last_route=route.value, kernel_ms=ms.value)

    def cancel(self):
        _lib.check(self.lib.tsq_unionstore_cancel(self.h), self.h)

    def close(self):
        if self.h:
            self.lib.tsq_unionstore_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()
