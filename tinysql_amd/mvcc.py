"""The MVCC snapshot read over libtsq (tsq_mvcc_*; include/tsq.h "MVCC snapshot read"): a versioned store in HBM and the reference's
Scan / ReverseScan / Get over key ranges at a startTS (store/mockstore/mocktikv/mvcc_leveldb.go:261-430).  Everything below is plumbing
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

    def free(self):
        for a in (self.keys, self.key_offsets, self.values, self.value_offsets):
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

    def __init__(self, ctx, data, device=False):
        self.ctx, self.lib, self.h = ctx, ctx.lib, None
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
        _lib.check(self.lib.tsq_mvcc_create(ctx.h, C.byref(d), C.byref(h)), ctx.h)
        self.h = h
        self.n, self.n_locks = d.n, d.n_locks

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
