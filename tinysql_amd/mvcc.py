"""The MVCC store over libtsq (tsq_mvcc_*; include/tsq.h "MVCC snapshot read", "MVCC writes", "MVCC lock resolution and GC"): a versioned
store in HBM, the reference's Scan / ReverseScan / Get over key ranges at a startTS (store/mockstore/mocktikv/mvcc_leveldb.go:261-430),
its Prewrite / Commit / Rollback (:442-717) and its ScanLock / ResolveLock / BatchResolveLock / GC / DeleteRange (:906-1090) into the
next store — a new MvccStore; the one a call was made on stays readable.  Everything below is plumbing
around the C-ABI; the pairs of a read stay on the device, in the keys / offsets / values / offsets form the scan executors decode."""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib
from .dupcheck import DevArray

U64_MAX = (1 << 64) - 1


def mvccEncode(key, ver):
    """codec.EncodeBytes(key) + codec.EncodeUintDesc(ver) (mvcc.go mvccEncode)"""
    out = bytearray()
    for i in range(0, len(key) + 1, 8):
        g = key[i:i + 8]
        pad = 8 - len(g)
        out += g + b"\x00" * pad + bytes([0xFF - pad])
    return bytes(out) + ((~ver) & U64_MAX).to_bytes(8, "big")


class ErrLocked(_lib.TsqError):
    """mocktikv.ErrLocked as lockErr builds it (mvcc.go:187-195): Key = mvccEncode(raw key, lockVer)"""

    def __init__(self, raw_key, primary, start_ts, ttl, op):
        _lib.TsqError.__init__(self, abi.ERR_LOCKED, "key is locked, key: %r, primary: %r, startTS: %d" % (raw_key, primary, start_ts))
        self.RawKey = raw_key
        self.Key, self.Primary, self.StartTS, self.TTL, self.LockType = mvccEncode(raw_key, U64_MAX), primary, start_ts, ttl, op


class WriteError(Exception):
    """an error of Prewrite / Commit / Rollback.  The exception a write raises is the reference's — the error of the first failing key
    — and carries `errors`: one entry per mutation / key of the call, in the caller's order, None or that key's exception (Prewrite
    returns exactly this list, mvcc_leveldb.go:452-464)"""
    errors = ()


class ErrConflict(WriteError):
    """mocktikv.ErrConflict (mvcc_leveldb.go:482-489)"""

    def __init__(self, start_ts, conflict_ts, conflict_commit_ts, key):
        WriteError.__init__(self, "write conflict, startTS: %d, conflictTS: %d, conflictCommitTS: %d, key: %r" % (start_ts, conflict_ts, conflict_commit_ts, key))
        self.StartTS, self.ConflictTS, self.ConflictCommitTS, self.Key = start_ts, conflict_ts, conflict_commit_ts, key


class ErrRetryable(WriteError):
    """mocktikv.ErrRetryable("txn not found") (mvcc_leveldb.go:581)"""

    def __init__(self, key, message="txn not found"):
        WriteError.__init__(self, "retryable: %s" % message)
        self.Key, self.Message = key, message


class ErrAlreadyCommitted(WriteError):
    """mocktikv.ErrAlreadyCommitted(commitTS) (mvcc_leveldb.go:664)"""

    def __init__(self, key, commit_ts):
        WriteError.__init__(self, "txn already committed, commitTS: %d" % commit_ts)
        self.Key, self.CommitTS = key, commit_ts


class ErrGCLocked(WriteError):
    """GC's refusal (mvcc_leveldb.go:1041-1047): a lock of the range has startTS <= safePoint; the first such lock in key order"""

    def __init__(self, key, start_ts, safe_point):
        WriteError.__init__(self, "key %r has lock with startTs %d which is under safePoint %d" % (key, start_ts, safe_point))
        self.Key, self.StartTS, self.SafePoint = key, start_ts, safe_point


class LockInfo:
    """kvrpcpb.LockInfo as ScanLock fills it (mvcc_leveldb.go:924-928), plus the lock's index among the store's sorted lock keys"""

    def __init__(self, primary, version, key, index=-1):
        self.PrimaryLock, self.LockVersion, self.Key, self.Index = primary, version, key, index

    def fields(self):
        return (self.PrimaryLock, self.LockVersion, self.Key)

    def __eq__(self, other):
        return isinstance(other, LockInfo) and self.fields() == other.fields()

    def __repr__(self):
        return "LockInfo(%r, %d, %r)" % self.fields()


def _host_bytes(b):
    a = np.frombuffer(bytes(b), dtype=np.uint8).copy()
    return a, (a.ctypes.data if a.size else None), a.size


def _pack_cells(cells):
    offs = np.zeros(len(cells) + 1, dtype=np.int64)
    if cells:
        offs[1:] = np.cumsum([len(c) for c in cells])
    return np.frombuffer(b"".join(cells), dtype=np.uint8).copy(), offs


class Pairs:
    """the pairs of one read, device resident: keys back to back with n + 1 offsets, values back to back with n + 1 offsets; counts =
    the pairs of every range (after the limit)"""

    def __init__(self, ctx, n, key_bytes, value_bytes, counts, positions):
        self.ctx, self.n, self.key_bytes, self.value_bytes, self.counts, self.positions = ctx, n, key_bytes, value_bytes, counts, positions
        self.keys, self.key_offsets = DevArray(ctx, nbytes=key_bytes + 8), DevArray(ctx, nbytes=(n + 1) * 8)
        self.values, self.value_offsets = DevArray(ctx, nbytes=value_bytes + 8), DevArray(ctx, nbytes=(n + 1) * 8)

    def to_host(self):
        """[(key, value)] — for tests and small reads"""
        ko, vo = self.key_offsets.read(np.int64, self.n + 1), self.value_offsets.read(np.int64, self.n + 1)
        kb, vb = self.keys.read(np.uint8, self.key_bytes).tobytes(), self.values.read(np.uint8, self.value_bytes).tobytes()
        return [(kb[ko[i]:ko[i + 1]], vb[vo[i]:vo[i + 1]]) for i in range(self.n)]

    def release_values(self):
        """hands the values and their offsets (two DevArrays) over to the caller, who frees them; free() then frees what is left"""
        out = (self.values, self.value_offsets)
        self.values = self.value_offsets = None
        return out

    def free(self):
        for a in (self.keys, self.key_offsets, self.values, self.value_offsets):
            if a is not None:
                a.free()


def pack_ranges(ranges):
    """[(start, end)] — end None: the point Get(start) — -> (range bytes, 2 n + 1 offsets, n flags), what tsq_mvcc_scan takes"""
    parts, offs, flags = [], [0], []
    for start, end in ranges:
        point = end is None
        for b in (start, b"" if point else end):
            parts.append(b)
            offs.append(offs[-1] + len(b))
        flags.append(abi.MVCC_POINT if point else 0)
    return (np.frombuffer(b"".join(parts), dtype=np.uint8).copy(), np.array(offs, dtype=np.int64), np.array(flags, dtype=np.uint32))


class MvccStore:
    """tsq_mvcc: the store's versions and locks, uploaded once.  `data` maps the field names of tsq_mvcc_data to numpy arrays (host), or
    with device=True to (device pointer, element count) pairs."""

    FIELDS = (("keys", "key_bytes"), ("key_offsets", None), ("commit_ts", None), ("start_ts", None), ("types", None), ("values", "value_bytes"),
              ("value_offsets", None), ("lock_keys", "lock_key_bytes"), ("lock_key_offsets", None), ("lock_start_ts", None), ("lock_ttl", None),
              ("lock_ops", None), ("lock_primaries", "lock_primary_bytes"), ("lock_primary_offsets", None))
    DTYPES = dict(keys=np.uint8, key_offsets=np.int64, commit_ts=np.uint64, start_ts=np.uint64, types=np.uint8, values=np.uint8, value_offsets=np.int64,
                  lock_keys=np.uint8, lock_key_offsets=np.int64, lock_start_ts=np.uint64, lock_ttl=np.uint64, lock_ops=np.uint8, lock_primaries=np.uint8,
                  lock_primary_offsets=np.int64)

    RW_FIELDS = (("lock_values", np.uint8), ("lock_value_offsets", np.int64))

    def __init__(self, ctx, data, device=False, rw=False):
        """rw: a writable store (tsq_mvcc_create_rw) — data also holds start_ts, lock_values and lock_value_offsets"""
        self.ctx, self.lib, self.h = ctx, ctx.lib, None
        self.rw, self.last_write = rw, None
        d = abi.MvccData()
        keep = []
        counts = {}
        for name, size_field in self.FIELDS:
            v = data.get(name)
            if v is None:
                counts[name] = 0
                continue
            if device:
                p, cnt = v
            else:
                v = np.ascontiguousarray(v, dtype=self.DTYPES[name])
                keep.append(v)
                p, cnt = (v.ctypes.data if v.size else None), v.size
            setattr(d, name, p)
            counts[name] = cnt
            if size_field:
                setattr(d, size_field, cnt)
        d.n = max(counts["key_offsets"] - 1, 0)
        d.n_locks = max(counts["lock_key_offsets"] - 1, 0)
        d.data_flags = abi.COL_DEVICE if device else 0
        h = C.c_void_p()
        if rw:
            lv, lo = data.get("lock_values"), data.get("lock_value_offsets")
            if device:
                (lvp, lvn), lop = (lv if lv is not None else (None, 0)), (lo[0] if lo is not None else None)
            else:
                lv = np.ascontiguousarray(lv if lv is not None else [], dtype=np.uint8)
                lo = np.ascontiguousarray(lo if lo is not None else [0], dtype=np.int64)
                keep += [lv, lo]
                lvp, lvn, lop = (lv.ctypes.data if lv.size else None), lv.size, lo.ctypes.data
            _lib.check(self.lib.tsq_mvcc_create_rw(ctx.h, C.byref(d), C.c_void_p(lvp), C.c_void_p(lop), lvn, C.byref(h)), ctx.h)
        else:
            _lib.check(self.lib.tsq_mvcc_create(ctx.h, C.byref(d), C.byref(h)), ctx.h)
        self.h = h
        self.n, self.n_locks = d.n, d.n_locks

    @classmethod
    def create_rw(cls, ctx, data, device=False):
        """a writable store: `data` as for a plain one plus start_ts (required), lock_values and lock_value_offsets"""
        return cls(ctx, data, device, rw=True)

    @classmethod
    def _next(cls, ctx, h, res):
        s = cls.__new__(cls)
        s.ctx, s.lib, s.h, s.rw = ctx, ctx.lib, h, True
        s.last_write = {k: getattr(res, k) for k, _ in abi.MvccWriteResult._fields_}
        z = s.sizes()
        s.n, s.n_locks = z["n"], z["n_locks"]
        return s

    # ------------------------------------------------------------------ the writes (include/tsq.h "MVCC writes")
    def write_packed(self, kind, req, n):
        """one call of tsq_mvcc_prewrite / commit / rollback over a filled abi.MvccWriteReq (keys strictly ascending; host or device
        arrays) -> (the next MvccStore or None, verdict bytes, info [n, 2], result).  Raises only what the C-ABI refuses."""
        fn = {"prewrite": self.lib.tsq_mvcc_prewrite, "commit": self.lib.tsq_mvcc_commit, "rollback": self.lib.tsq_mvcc_rollback}[kind]
        verdicts, info = np.zeros(max(n, 1), dtype=np.uint8), np.zeros((max(n, 1), 2), dtype=np.uint64)
        res, nxt = abi.MvccWriteResult(), C.c_void_p()
        _lib.check(fn(self.h, C.byref(req), verdicts.ctypes.data, info.ctypes.data, C.byref(res), C.byref(nxt)), self.h)
        store = MvccStore._next(self.ctx, nxt, res) if nxt.value else None
        return store, verdicts[:n], info[:n], res

    def _write(self, kind, keys, ops, values, primary, start_ts, commit_ts, ttl):
        """the host mirror: sorts the keys, drops duplicates (the last one wins), maps the verdicts back to the caller's order"""
        last = {}
        for i, k in enumerate(keys):
            last[bytes(k)] = i
        order = sorted(last.values(), key=lambda i: bytes(keys[i]))
        kb, ko = _pack_cells([bytes(keys[i]) for i in order])
        req = abi.MvccWriteReq()
        req.keys, req.key_offsets, req.key_bytes, req.n_keys = (kb.ctypes.data if kb.size else None), ko.ctypes.data, kb.size, len(order)
        if kind == "prewrite":
            o = np.array([ops[i] for i in order], dtype=np.uint8)
            vb, vo = _pack_cells([bytes(values[i]) for i in order])
            pr = np.frombuffer(bytes(primary), dtype=np.uint8).copy()
            req.ops, req.values, req.value_offsets, req.value_bytes = (o.ctypes.data if o.size else None), (vb.ctypes.data if vb.size else None), vo.ctypes.data, vb.size
            req.primary, req.primary_len = (pr.ctypes.data if pr.size else None), pr.size
        req.start_ts, req.commit_ts, req.ttl = start_ts, commit_ts, ttl
        store, verdicts, info, res = self.write_packed(kind, req, len(order))
        if store is not None:
            return store
        slot = {bytes(keys[i]): j for j, i in enumerate(order)}
        errors = [self._key_error(bytes(k), int(verdicts[slot[bytes(k)]]), info[slot[bytes(k)]], start_ts) for k in keys]
        first = self._key_error(bytes(keys[order[res.first_error]]), int(verdicts[res.first_error]), info[res.first_error], start_ts)
        first.errors = errors
        raise first

    def _key_error(self, key, verdict, info, start_ts):
        if verdict == abi.MVCC_V_LOCKED:
            return self.lock_at(int(info[0]))
        if verdict == abi.MVCC_V_CONFLICT:
            return ErrConflict(start_ts, int(info[0]), int(info[1]), key)
        if verdict == abi.MVCC_V_TXN_NOT_FOUND:
            return ErrRetryable(key)
        if verdict == abi.MVCC_V_ALREADY_COMMITTED:
            return ErrAlreadyCommitted(key, int(info[0]))
        return None

    def prewrite(self, mutations, primary, start_ts, ttl=0):
        """Prewrite: mutations = [(op, key, value)] (abi.MVCC_OP_PUT / DEL / LOCK) -> the next MvccStore; raises ErrLocked / ErrConflict
        with .errors, the per-mutation list"""
        return self._write("prewrite", [m[1] for m in mutations], [m[0] for m in mutations], [m[2] for m in mutations], primary, start_ts, 0, ttl)

    def commit(self, keys, start_ts, commit_ts):
        """Commit -> the next MvccStore; raises ErrRetryable("txn not found") with .errors"""
        return self._write("commit", list(keys), None, None, None, start_ts, commit_ts, 0)

    def rollback(self, keys, start_ts):
        """Rollback -> the next MvccStore; raises ErrAlreadyCommitted with .errors"""
        return self._write("rollback", list(keys), None, None, None, start_ts, 0, 0)

    # ------------------------------------------------------------------ the range calls (include/tsq.h "MVCC lock resolution and GC")
    def scan_lock_packed(self, start, end, max_ts, device=False):
        """tsq_mvcc_scan_lock + fetch -> (n, keys, key offsets, primaries, primary offsets, start_ts, lock indexes): numpy arrays, or
        with device=True DevArrays the caller frees"""
        res = abi.MvccLockScan()
        sa, sp, sn = _host_bytes(start)
        ea, ep, en = _host_bytes(end)
        _lib.check(self.lib.tsq_mvcc_scan_lock(self.h, sp, sn, ep, en, C.c_uint64(max_ts), C.byref(res)), self.h)
        n, kb, pb = res.n_locks, res.key_bytes, res.primary_bytes
        sizes = (kb + 8, (n + 1) * 8, pb + 8, (n + 1) * 8, n * 8 + 8, n * 8 + 8)
        dtypes = (np.uint8, np.int64, np.uint8, np.int64, np.uint64, np.int64)
        if device:
            out = [DevArray(self.ctx, nbytes=z) for z in sizes]
            ptrs = [C.c_void_p(a.p) for a in out]
        else:
            out = [np.zeros(z // np.dtype(t).itemsize, dtype=t) for z, t in zip(sizes, dtypes)]
            ptrs = [C.c_void_p(a.ctypes.data) for a in out]
        try:
            _lib.check(self.lib.tsq_mvcc_scan_lock_fetch(self.h, ptrs[0], kb, ptrs[1], ptrs[2], pb, ptrs[3], ptrs[4], ptrs[5], abi.COL_DEVICE if device else 0),
                       self.h)
        except _lib.TsqError:
            if device:
                for a in out:
                    a.free()
            raise
        self.last_scan_lock = {k: getattr(res, k) for k, _ in abi.MvccLockScan._fields_}
        return (n,) + tuple(out)

    def scan_lock(self, start, end, max_ts):
        """ScanLock -> [LockInfo] in key order: the locks of [start, end) with startTS <= max_ts"""
        n, keys, ko, prims, po, sts, idx = self.scan_lock_packed(start, end, max_ts)
        kb, pb = keys.tobytes(), prims.tobytes()
        return [LockInfo(pb[po[i]:po[i + 1]], int(sts[i]), kb[ko[i]:ko[i + 1]], int(idx[i])) for i in range(n)]

    def _maint(self, fn, start, end, *mid):
        sa, sp, sn = _host_bytes(start)
        ea, ep, en = _host_bytes(end)
        res, nxt = abi.MvccMaintResult(), C.c_void_p()
        _lib.check(fn(self.h, sp, sn, ep, en, *(mid + (C.byref(res), C.byref(nxt)))), self.h)
        self.last_maint = {k: getattr(res, k) for k, _ in abi.MvccMaintResult._fields_}
        if not nxt.value:
            return self, res
        s = MvccStore.__new__(MvccStore)
        s.ctx, s.lib, s.h, s.rw, s.last_write = self.ctx, self.lib, nxt, True, None
        s.last_maint = self.last_maint
        z = s.sizes()
        s.n, s.n_locks = z["n"], z["n_locks"]
        return s, res

    def batch_resolve_lock(self, start, end, txn_infos):
        """BatchResolveLock: txn_infos = {start_ts: commit_ts} (or pairs; commit_ts 0 rolls back) -> the next MvccStore, or self when
        no lock matched"""
        pairs = list(txn_infos.items()) if isinstance(txn_infos, dict) else [(int(a), int(b)) for a, b in txn_infos]
        st = np.array([p[0] for p in pairs], dtype=np.uint64)
        ct = np.array([p[1] for p in pairs], dtype=np.uint64)
        return self._maint(self.lib.tsq_mvcc_resolve_lock, start, end, st.ctypes.data if st.size else None, ct.ctypes.data if ct.size else None, len(pairs))[0]

    def resolve_lock(self, start, end, start_ts, commit_ts):
        """ResolveLock: commit (commit_ts > 0) or roll back every lock of start_ts in the range -> the next MvccStore, or self"""
        return self.batch_resolve_lock(start, end, [(start_ts, commit_ts)])

    def gc(self, start, end, safe_point):
        """GC -> the next MvccStore, or self when nothing was at or under the safe point; raises ErrGCLocked"""
        s, res = self._maint(self.lib.tsq_mvcc_gc, start, end, C.c_uint64(safe_point))
        if res.n_errors:
            l = self.lock_at(res.first_error)
            raise ErrGCLocked(l.RawKey, l.StartTS, safe_point)
        return s

    def delete_range(self, start, end):
        """DeleteRange: every version and lock of start <= key < end goes; an EMPTY end deletes nothing -> the next MvccStore, or self"""
        return self._maint(self.lib.tsq_mvcc_delete_range, start, end)[0]

    def lock_at(self, j):
        """lock j as the ErrLocked lockErr builds for it (tsq_mvcc_lock_at)"""
        kl, pl, ts, ttl, op = C.c_int64(0), C.c_int64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        st = self.lib.tsq_mvcc_lock_at(self.h, j, None, 0, C.byref(kl), None, 0, C.byref(pl), C.byref(ts), C.byref(ttl), C.byref(op))
        if st not in (abi.OK, abi.ERR_INVALID) or (st == abi.ERR_INVALID and kl.value == 0 and pl.value == 0):
            _lib.check(st, self.h)
        key, prim = np.zeros(max(kl.value, 1), dtype=np.uint8), np.zeros(max(pl.value, 1), dtype=np.uint8)
        _lib.check(self.lib.tsq_mvcc_lock_at(self.h, j, key.ctypes.data, kl.value, C.byref(kl), prim.ctypes.data, pl.value, C.byref(pl), C.byref(ts), C.byref(ttl),
                                             C.byref(op)), self.h)
        return ErrLocked(key[:kl.value].tobytes(), prim[:pl.value].tobytes(), ts.value, ttl.value, op.value)

    def sizes(self):
        z = abi.MvccStoreSizes()
        _lib.check(self.lib.tsq_mvcc_sizes(self.h, C.byref(z)), self.h)
        return {k: getattr(z, k) for k, _ in abi.MvccStoreSizes._fields_}

    def export_device(self):
        """every array of a writable store in HBM: {name: DevArray} (tsq_mvcc_arrays' names) and the sizes; the caller frees them"""
        z = self.sizes()
        n, nl = z["n"], z["n_locks"]
        nbytes = dict(keys=z["key_bytes"], key_offsets=(n + 1) * 8, commit_ts=n * 8, start_ts=n * 8, types=n, values=z["value_bytes"], value_offsets=(n + 1) * 8,
                      lock_keys=z["lock_key_bytes"], lock_key_offsets=(nl + 1) * 8, lock_start_ts=nl * 8, lock_ttl=nl * 8, lock_ops=nl,
                      lock_primaries=z["lock_primary_bytes"], lock_primary_offsets=(nl + 1) * 8, lock_values=z["lock_value_bytes"], lock_value_offsets=(nl + 1) * 8)
        arrs = {name: DevArray(self.ctx, nbytes=nbytes[name]) for name in abi.MVCC_ARRAY_NAMES}
        a = abi.MvccArrays()
        for name in abi.MVCC_ARRAY_NAMES:
            setattr(a, name, arrs[name].p)
        try:
            _lib.check(self.lib.tsq_mvcc_export(self.h, C.byref(a)), self.h)
        except _lib.TsqError:
            for d in arrs.values():
                d.free()
            raise
        return arrs, z

    def export(self):
        """the store as host numpy arrays, under the names MvccStore.create_rw takes"""
        arrs, z = self.export_device()
        dtypes = dict(self.DTYPES, lock_values=np.uint8, lock_value_offsets=np.int64)
        try:
            return {name: arrs[name].read(dtypes[name], arrs[name].nbytes // np.dtype(dtypes[name]).itemsize) for name in abi.MVCC_ARRAY_NAMES}
        finally:
            for d in arrs.values():
                d.free()

    def scan_packed(self, range_bytes, range_offsets, range_flags, start_ts, desc=False, limit=None, fetch=True):
        """the read over packed ranges (pack_ranges) -> Pairs (fetch=False: only the counts; Pairs.keys etc. stay unwritten)"""
        n_ranges = len(range_offsets) // 2
        res = abi.MvccResult()
        counts = np.zeros(max(n_ranges, 1), dtype=np.int64)
        st = self.lib.tsq_mvcc_scan(self.h, range_bytes.ctypes.data if range_bytes.size else None, range_offsets.ctypes.data,
                                    range_flags.ctypes.data if range_flags is not None and range_flags.size else None, n_ranges, C.c_uint64(start_ts),
                                    1 if desc else 0, -1 if limit is None else limit, C.byref(res), counts.ctypes.data)
        if st == abi.ERR_LOCKED:
            raise self._locked()
        _lib.check(st, self.h)
        out = Pairs(self.ctx, res.n_pairs, res.key_bytes, res.value_bytes, counts[:n_ranges].tolist(), res.positions)
        if fetch:
            try:
                _lib.check(self.lib.tsq_mvcc_fetch(self.h, C.c_void_p(out.keys.p), res.key_bytes, C.c_void_p(out.key_offsets.p), C.c_void_p(out.values.p),
                                                   res.value_bytes, C.c_void_p(out.value_offsets.p)), self.h)
            except _lib.TsqError:
                out.free()
                raise
        return out

    def scan(self, ranges, start_ts, desc=False, limit=None):
        """Scan / ReverseScan of the ranges in the order given ((start, end); (start, None) = Get(start)) at start_ts; raises ErrLocked"""
        rb, ro, rf = pack_ranges(ranges)
        return self.scan_packed(rb, ro, rf, start_ts, desc, limit)

    def get(self, key, ts):
        """Get: the value or None; raises ErrLocked"""
        p = self.scan([(key, None)], ts)
        try:
            got = p.to_host()
        finally:
            p.free()
        return got[0][1] if got else None

    def _locked(self):
        kl, pl, ts, ttl, op = C.c_int64(0), C.c_int64(0), C.c_uint64(0), C.c_uint64(0), C.c_int32(0)
        st = self.lib.tsq_mvcc_locked(self.h, None, 0, C.byref(kl), None, 0, C.byref(pl), C.byref(ts), C.byref(ttl), C.byref(op))
        if st not in (abi.OK, abi.ERR_INVALID) or (st == abi.ERR_INVALID and kl.value == 0 and pl.value == 0):
            _lib.check(st, self.h)
        key, prim = np.zeros(max(kl.value, 1), dtype=np.uint8), np.zeros(max(pl.value, 1), dtype=np.uint8)
        _lib.check(self.lib.tsq_mvcc_locked(self.h, key.ctypes.data, kl.value, C.byref(kl), prim.ctypes.data, pl.value, C.byref(pl), C.byref(ts), C.byref(ttl),
                                            C.byref(op)), self.h)
        return ErrLocked(key[:kl.value].tobytes(), prim[:pl.value].tobytes(), ts.value, ttl.value, op.value)

    def stats(self):
        a, b, c, d, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_mvcc_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(d), C.byref(ms)), self.h)
        return {"scans": a.value, "keys_examined": b.value, "versions_read": c.value, "pairs": d.value, "kernel_ms": ms.value}

    def cancel(self):
        _lib.check(self.lib.tsq_mvcc_cancel(self.h), self.h)

    def close(self):
        if self.h:
            self.lib.tsq_mvcc_destroy(self.h)
            self.h = None


def insert_batch_mutations(batch):
    """the record keys (19 bytes each) and stored rows of a gpu_pipeline.InsertBatch as the Put mutations of a device-resident prewrite
    request: the key and value bytes stay where they are in HBM; only the key offsets and the ops, which the batch does not hold, are
    made on the host and uploaded (9 bytes per row).  Record keys of ascending handles are ascending keys; the order check of the
    prewrite is the check.  -> (abi.MvccWriteReq without primary / timestamps, [DevArray to free after the call])"""
    n = batch.n
    koff, ops = DevArray(batch.ctx, np.arange(n + 1, dtype=np.int64) * 19), DevArray(batch.ctx, np.zeros(max(n, 1), dtype=np.uint8))
    req = abi.MvccWriteReq()
    req.keys, req.key_offsets, req.key_bytes, req.n_keys = batch.row_keys, koff.p, n * 19, n
    req.ops, req.values, req.value_offsets, req.value_bytes = ops.p, batch.row_values.p, batch.row_values.offsets, batch.row_values.nbytes
    req.flags = abi.COL_DEVICE
    return req, [koff, ops]


def write_insert_batches(store, batches, primary, start_ts, commit_ts, ttl=0):
    """prewrites and commits the row stream of a statement (the InsertBatches of GpuInsertSelectExec over a table without secondary
    indexes) and returns the next store; `store` stays as it is and the intermediate stores are closed.  Each batch's handles ascend
    and the batches do not overlap in key order, or the prewrite answers "keys not strictly ascending".  Index streams of a table
    with secondary indexes need a key sort: they go through the transaction buffer (kv.MemBuffer, InsertBatch.write_to, then
    write_membuffer below).  Raises ErrLocked / ErrConflict (with .errors, per row of the failing batch); nothing of the statement is
    then visible in `store`."""
    cur = store
    pr = np.frombuffer(bytes(primary), dtype=np.uint8).copy()

    def step(kind, req, n):
        nonlocal cur
        nxt, verdicts, info, res = cur.write_packed(kind, req, n)
        if nxt is None:
            at = res.first_error
            ko = np.zeros(2, dtype=np.int64)
            cur.ctx.d2h(ko, req.key_offsets + 8 * at)
            key = np.zeros(max(int(ko[1] - ko[0]), 1), dtype=np.uint8)
            cur.ctx.d2h(key, req.keys + int(ko[0]))
            key = key[:int(ko[1] - ko[0])].tobytes()
            err = cur._key_error(key, int(verdicts[at]), info[at], start_ts)
            err.errors = [None if v < abi.MVCC_V_LOCKED else (err if i == at else int(v)) for i, v in enumerate(verdicts)]
            if cur is not store:
                cur.close()
            raise err
        if cur is not store:
            cur.close()
        cur = nxt

    for kind in ("prewrite", "commit"):
        for b in batches:
            req, tmp = insert_batch_mutations(b)
            try:
                req.primary, req.primary_len = (pr.ctypes.data if pr.size else None), pr.size
                req.start_ts, req.commit_ts, req.ttl = start_ts, commit_ts, ttl
                step(kind, req, b.n)
            finally:
                for t in tmp:
                    t.free()
    return cur


def _request_key(ctx, req, at):
    """key `at` of a device-resident request, read back (two offsets, then its bytes)"""
    ko = np.zeros(2, dtype=np.int64)
    ctx.d2h(ko, req.key_offsets + 8 * at)
    key = np.zeros(max(int(ko[1] - ko[0]), 1), dtype=np.uint8)
    ctx.d2h(key, req.keys + int(ko[0]))
    return key[:int(ko[1] - ko[0])].tobytes()


def write_membuffer(store, membuf, start_ts, commit_ts, ttl=0, primary=None):
    """prewrites and commits a whole transaction buffer (kv.MemBuffer) as ONE device-resident request — the buffer's own sorted arrays,
    no key or value byte crosses to the host — and returns the next store; `store` stays as it is and the intermediate store is
    closed.  primary None: the buffer's own (the reference's c.keys[0]), read back from the request.  Raises what
    write_insert_batches raises, with the key read back from the request; nothing of the transaction is then visible in `store`."""
    res = membuf.finish()
    req = membuf.request()
    n = req.n_keys
    if n == 0:
        return store
    if primary is None:
        primary = _request_key(store.ctx, req, res["primary_index"])
    pr = np.frombuffer(bytes(primary), dtype=np.uint8).copy()
    req.primary, req.primary_len = (pr.ctypes.data if pr.size else None), pr.size
    req.start_ts, req.commit_ts, req.ttl = start_ts, commit_ts, ttl
    cur = store
    for kind in ("prewrite", "commit"):
        nxt, verdicts, info, wres = cur.write_packed(kind, req, n)
        if nxt is None:
            at = wres.first_error
            err = cur._key_error(_request_key(store.ctx, req, at), int(verdicts[at]), info[at], start_ts)
            err.errors = [None if v < abi.MVCC_V_LOCKED else (err if i == at else int(v)) for i, v in enumerate(verdicts)]
            if cur is not store:
                cur.close()
            raise err
        if cur is not store:
            cur.close()
        cur = nxt
    return cur
