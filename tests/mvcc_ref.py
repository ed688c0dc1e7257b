"""The sequential model of the MVCC store's read side (store/mockstore/mocktikv): getValue (mvcc_leveldb.go:280-312), Scan and
ReverseScan (:315-430), Get (:263-268), mvccLock.check (mvcc.go:197-207) and mvccEntry.Get (mvcc.go:213-227), restated plainly over
a dict of version lists and a dict of locks — plus, for the host only, the write side the reference's tests build their states with
(Prewrite, Commit, Rollback: mvcc_leveldb.go:493-700).  tests/golden/mvcc_cases.json holds it to the reference's own vectors; the
GPU tests hold tsq_mvcc_* to it."""
import bisect
from collections import namedtuple

import numpy as np

PUT, DELETE, ROLLBACK = 0, 1, 2  # typePut, typeDelete, typeRollback (mvcc.go:30-34)
OP_PUT, OP_DEL, OP_LOCK, OP_ROLLBACK = 0, 1, 2, 3  # kvrpcpb.Op
OP_NAMES = {"put": OP_PUT, "del": OP_DEL, "lock": OP_LOCK, "rollback": OP_ROLLBACK}
U64_MAX = (1 << 64) - 1
LOCK_VER = U64_MAX
NO_LIMIT = 1 << 62

Value = namedtuple("Value", "type start_ts commit_ts value")
Lock = namedtuple("Lock", "start_ts primary value op ttl")


def encode_bytes(b):
    """codec.EncodeBytes: groups of 8 bytes, zero padded, each followed by 0xFF - pad."""
    out = bytearray()
    for i in range(0, len(b) + 1, 8):
        g = b[i:i + 8]
        pad = 8 - len(g)
        out += g + b"\x00" * pad + bytes([0xFF - pad])
    return bytes(out)


def mvcc_encode(key, ver):
    """mvccEncode: EncodeBytes(key) + EncodeUintDesc(ver)."""
    return encode_bytes(key) + ((~ver) & U64_MAX).to_bytes(8, "big")


class ErrLocked(Exception):
    def __init__(self, key, lock):
        Exception.__init__(self, "key is locked")
        self.RawKey = key
        self.Key = mvcc_encode(key, LOCK_VER)  # lockErr (mvcc.go:187-195)
        self.Primary, self.StartTS, self.TTL, self.LockType = lock.primary, lock.start_ts, lock.ttl, lock.op

    def fields(self):
        return (self.Key, self.Primary, self.StartTS, self.TTL, self.LockType)


class WriteError(Exception):
    pass


def lock_check(lock, ts, key):
    """mvccLock.check: the ts the read goes on at, or ErrLocked."""
    if lock.start_ts > ts or lock.op == OP_LOCK:
        return ts
    if ts == U64_MAX and lock.primary == key:
        return (lock.start_ts - 1) & U64_MAX
    raise ErrLocked(key, lock)


class Store:
    def __init__(self):
        self.versions = {}  # key -> [Value], descending commit_ts
        self.locks = {}  # key -> Lock
        self._keys = None  # freeze(): the sorted keys, kept for the many reads of a test

    # ------------------------------------------------------------------ the write side (host only)
    def _insert(self, key, v):
        vs = self.versions.setdefault(key, [])
        at = 0
        while at < len(vs) and vs[at].commit_ts > v.commit_ts:
            at += 1
        if at < len(vs) and vs[at].commit_ts == v.commit_ts:
            vs[at] = v  # one LevelDB key per (key, ver)
        else:
            vs.insert(at, v)

    def prewrite(self, mutations, primary, start_ts, ttl=0):
        for op, key, value in mutations:
            lock = self.locks.get(key)
            if lock is not None:
                if lock.start_ts != start_ts:
                    raise ErrLocked(key, lock)
            else:
                vs = self.versions.get(key, [])
                if vs and vs[0].commit_ts >= start_ts:
                    raise WriteError("write conflict")
            self.locks[key] = Lock(start_ts, primary, value, op, ttl)

    def commit(self, keys, start_ts, commit_ts):
        for key in keys:
            lock = self.locks.get(key)
            if lock is None or lock.start_ts != start_ts:
                c = [v for v in self.versions.get(key, []) if v.start_ts == start_ts]
                if c and c[0].type != ROLLBACK:
                    continue
                raise WriteError("txn not found")
            if lock.op != OP_LOCK:
                self._insert(key, Value(PUT if lock.op == OP_PUT else DELETE, start_ts, commit_ts, lock.value))
            del self.locks[key]

    def rollback(self, keys, start_ts):
        for key in keys:
            lock = self.locks.get(key)
            if lock is not None and lock.start_ts == start_ts:
                del self.locks[key]
                self._insert(key, Value(ROLLBACK, start_ts, start_ts, b""))
                continue
            c = [v for v in self.versions.get(key, []) if v.start_ts == start_ts]
            if c:
                if c[0].type != ROLLBACK:
                    raise WriteError("already committed")
                continue
            self._insert(key, Value(ROLLBACK, start_ts, start_ts, b""))

    def put(self, key, value, start_ts, commit_ts):  # mustPutOK
        self.prewrite([(OP_PUT, key, value)], key, start_ts)
        self.commit([key], start_ts, commit_ts)

    def delete(self, key, start_ts, commit_ts):  # mustDeleteOK
        self.prewrite([(OP_DEL, key, b"")], key, start_ts)
        self.commit([key], start_ts, commit_ts)

    # ------------------------------------------------------------------ the read side
    def keys(self):
        """every key the LevelDB iterator stops at: those with a version or a lock, ascending."""
        if self._keys is not None:
            return self._keys
        return sorted(set(self.versions) | set(self.locks))

    def freeze(self):
        """no write follows: keys() is computed once"""
        self._keys = sorted(set(self.versions) | set(self.locks))
        return self

    def get_value(self, key, ts):
        """getValue: the lock first, then the first version that is not a rollback and has commitTS <= ts."""
        lock = self.locks.get(key)
        if lock is not None:
            ts = lock_check(lock, ts, key)
        for v in self.versions.get(key, []):
            if v.type == ROLLBACK:
                continue
            if v.commit_ts <= ts:
                return None if v.type == DELETE else v.value
        return None

    def get(self, key, ts):
        return self.get_value(key, ts)

    def entry_get(self, key, ts):
        """mvccEntry.Get, as ReverseScan's finishEntry calls it: a delete's value is empty."""
        lock = self.locks.get(key)
        if lock is not None:
            ts = lock_check(lock, ts, key)
        for v in self.versions.get(key, []):
            if v.commit_ts <= ts and v.type != ROLLBACK:
                return v.value
        return None

    def _range(self, start, end):
        ks = self.keys()
        lo = bisect.bisect_left(ks, start) if start else 0
        hi = bisect.bisect_left(ks, end) if end else len(ks)
        return ks[lo:hi]

    def scan(self, start, end, limit, ts):
        """Scan: [(key, value, err)]; an error is a pair of its own and the scan goes on behind it."""
        pairs = []
        for key in self._range(start, end):
            if len(pairs) >= limit:
                break
            try:
                value = self.get_value(key, ts)
            except ErrLocked as e:
                pairs.append((key, None, e))
                continue
            if value is not None:
                pairs.append((key, value, None))
        return pairs

    def reverse_scan(self, start, end, limit, ts):
        pairs = []
        for key in reversed(self._range(start, end)):
            if len(pairs) >= limit:
                break
            try:
                value = self.entry_get(key, ts)
            except ErrLocked as e:
                pairs.append((key, None, e))
                continue
            if value:  # len(val) != 0
                pairs.append((key, value, None))
        return pairs

    # ------------------------------------------------------------------ the decoded LevelDB order tsq_mvcc_create takes
    def flat(self):
        keys, koff, cts, sts, types, vals, voff = [], [0], [], [], [], [], [0]
        for key in sorted(self.versions):
            for v in self.versions[key]:
                keys.append(key)
                koff.append(koff[-1] + len(key))
                cts.append(v.commit_ts)
                sts.append(v.start_ts)
                types.append(v.type)
                vals.append(v.value)
                voff.append(voff[-1] + len(v.value))
        lk = sorted(self.locks)
        locks = [self.locks[k] for k in lk]
        return flat_arrays(keys, cts, sts, types, vals, lk, [l.start_ts for l in locks], [l.ttl for l in locks], [l.op for l in locks],
                           [l.primary for l in locks])


def _pack(cells):
    offs = np.zeros(len(cells) + 1, dtype=np.int64)
    if cells:
        offs[1:] = np.cumsum([len(c) for c in cells])
    return np.frombuffer(b"".join(cells), dtype=np.uint8).copy(), offs


def flat_arrays(keys, cts, sts, types, vals, lock_keys, lock_start, lock_ttl, lock_ops, lock_prims):
    """the arrays of tsq_mvcc_data, as numpy (entries in the order given: a test may hand in a damaged order on purpose)."""
    kb, ko = _pack(keys)
    vb, vo = _pack(vals)
    lb, lo = _pack(lock_keys)
    pb, po = _pack(lock_prims)
    return dict(keys=kb, key_offsets=ko, commit_ts=np.array(cts, dtype=np.uint64), start_ts=np.array(sts, dtype=np.uint64),
                types=np.array(types, dtype=np.uint8), values=vb, value_offsets=vo, lock_keys=lb, lock_key_offsets=lo,
                lock_start_ts=np.array(lock_start, dtype=np.uint64), lock_ttl=np.array(lock_ttl, dtype=np.uint64),
                lock_ops=np.array(lock_ops, dtype=np.uint8), lock_primaries=pb, lock_primary_offsets=po)


def prefix_next(key):
    """kv.Key.PrefixNext: the smallest key greater than every key with this prefix."""
    b = bytearray(key)
    i = len(b) - 1
    while i >= 0:
        b[i] = (b[i] + 1) & 0xFF
        if b[i] != 0:
            break
        i -= 1
    if i == -1:
        return bytes(key) + b"\x00"
    return bytes(b)


def scan_ranges(kv_ranges, desc, points):
    """a request's KV ranges as read_ranges takes them, by the reference's rules and nothing of the product: with `points` (a table
    scan, executor.go:124-137; a UNIQUE index scan, executor.go:238) a range whose end is prefix_next(start) is Get(start); a
    non-unique index scans every range; desc walks the ranges from the last to the first (reverseKVRanges)"""
    rs = [(a, None) if points and b == prefix_next(a) else (a, b) for a, b in kv_ranges]
    return rs[::-1] if desc else rs


def read_ranges(store, ranges, ts, desc=False, limit=None):
    """what the scan executors read (executor.go:124-189, :271-320): the ranges in the order given — (start, end) or
    (start, None) for a point, Get(start) — the store asked per range with what is left of the limit, stopping at the first error.
    Returns (pairs, per-range counts); raises ErrLocked."""
    left = NO_LIMIT if limit is None or limit < 0 else limit
    pairs, counts = [], []
    for start, end in ranges:
        if end is None:
            got = []
            if left > 0 and start:
                v = store.get(start, ts)  # raises
                if v:  # len(val) == 0: no row
                    got = [(start, v, None)]
        elif desc:
            got = store.reverse_scan(start, end, left, ts)
        else:
            got = store.scan(start, end, left, ts)
        n = 0
        for key, value, err in got:
            if err is not None:
                raise err
            pairs.append((key, value))
            n += 1
        counts.append(n)
        left -= n
    return pairs, counts


# ---------------------------------------------------------------------- random stores (shared by the CPU and the GPU tests)
TS_ANCHORS = [0, 1, 5, 1000, (1 << 63) - 1, 1 << 63, (1 << 63) + 7, U64_MAX - 3, U64_MAX - 2]


def random_keys(rng, n, style):
    """n distinct keys.  'record': 19-byte record keys; 'prefix': 1..40 bytes over a two-letter alphabet with long shared prefixes,
    keys that are prefixes of one another included."""
    out = set()
    if style == "record":
        hs = rng.choice(1 << 20, n, replace=False)
        for h in hs:
            out.add(b"t" + (41 ^ (1 << 63)).to_bytes(8, "big") + b"_r" + (((int(h) - (1 << 19)) ^ (1 << 63)) & U64_MAX).to_bytes(8, "big"))
        return sorted(out)
    stem = bytes(rng.integers(65, 67, 34, dtype=np.uint8))
    while len(out) < n:
        ln = int(rng.integers(1, 41))
        if rng.random() < 0.5:
            k = stem[:min(ln, 34)] + bytes(rng.integers(0, 2, max(0, ln - 34), dtype=np.uint8))
        else:
            k = bytes(rng.integers(0, 3, min(ln, 12), dtype=np.uint8) + np.uint8(65))
        out.add(k)
        if rng.random() < 0.3 and len(k) < 40:
            out.add(k + b"\x00")
    return sorted(out)[:n] if len(out) > n else sorted(out)


def random_store(rng, n_keys, style="prefix", max_chain=5, lock_share=0.05, orphan_locks=2):
    s = Store()
    keys = random_keys(rng, n_keys, style)
    for key in keys:
        m = int(rng.integers(1, max_chain + 1))
        base = TS_ANCHORS[int(rng.integers(0, len(TS_ANCHORS)))]
        cts = set()
        while len(cts) < m:
            c = base + int(rng.integers(-40, 41))
            if 0 <= c <= U64_MAX - 1:
                cts.add(c)
        vs = []
        for c in sorted(cts, reverse=True):
            t = int(rng.choice([PUT, PUT, PUT, DELETE, ROLLBACK]))
            value = (b"v%d-" % c) + bytes(rng.integers(97, 123, int(rng.integers(0, 30)), dtype=np.uint8)) if t == PUT else b""
            vs.append(Value(t, max(0, c - 1), c, value))
        s.versions[key] = vs
    for key in keys:
        if rng.random() < lock_share:
            c = s.versions[key][int(rng.integers(0, len(s.versions[key])))].commit_ts
            st = min(U64_MAX, max(0, c + int(rng.integers(-2, 3))))
            prim = key if rng.random() < 0.5 else key + b"p"
            s.locks[key] = Lock(st, prim, b"x", int(rng.choice([OP_PUT, OP_DEL, OP_LOCK, OP_ROLLBACK])), int(rng.integers(0, 3000)))
    for i in range(orphan_locks):
        key = (keys[int(rng.integers(0, len(keys)))] if keys else b"K") + b"\x01o%d" % i
        s.locks[key] = Lock(int(rng.integers(0, 50)), key, b"y", OP_PUT, 7)
    return s


def read_timestamps(store, rng, n):
    """read timestamps around the store's own commitTS values and at the edges of uint64."""
    cts = [v.commit_ts for vs in store.versions.values() for v in vs] or [5]
    out = [0, 1, (1 << 63) - 1, 1 << 63, U64_MAX - 1, U64_MAX]
    for _ in range(n):
        c = cts[int(rng.integers(0, len(cts)))]
        out.append(min(U64_MAX, max(0, c + int(rng.integers(-1, 2)))))
    return out


def random_ranges(store, rng, n):
    """ranges over the store's keys: bounds on keys, between keys, before the first and after the last, empty bounds, start >= end,
    points that hit, miss, or are a proper prefix of a stored key; overlaps and repeats come by themselves."""
    ks = store.keys() or [b"m"]
    out = []

    def bound():
        k = ks[int(rng.integers(0, len(ks)))]
        w = rng.random()
        if w < 0.4:
            return k
        if w < 0.6:
            return k + b"\x00"
        if w < 0.75:
            return k[:-1] if len(k) > 1 else k
        if w < 0.85:
            return b"\x00" if rng.random() < 0.5 else b"\xff\xff"
        return b""
    for _ in range(n):
        w = rng.random()
        if w < 0.3:
            k = ks[int(rng.integers(0, len(ks)))]
            q = rng.random()
            out.append(((k if q < 0.5 else (k + b"!" if q < 0.75 else (k[:-1] or k))), None))
        else:
            out.append((bound(), bound()))
    if out and rng.random() < 0.5:
        out.append(out[0])
    return out
