"""Plain Python restatement of a transaction's merged read: kv.UnionIter (kv/union_iter.go: updateCur :64-137, Next :140-152),
BufferStore.Get / Iter / IterReverse (kv/buffer_store.go:61-99) — over the dict model of the transaction buffer (tests/membuf_ref.py,
tests/memread_ref.py) as the dirty side and the model of the versioned store (tests/mvcc_ref.py) as the snapshot side.

The snapshot iterator is the reference's scanner (store/tikv/scan.go:88-135) over mocktikv: it stands on visible pairs and FAILS when a
step takes it onto a locked key — at construction, on Next after a snapshot pair was yielded, and inside updateCur as soon as a buffer
key equals the snapshot key.  The consumer (`read`) takes pairs while Valid() and fewer than `limit` are taken, does not call Next
after the limit-th pair, and opens the next range only while the limit is not reached.

The host build of tsq_unionstore_dp.h and the GPU (tsq_unionstore_*) are held to this file."""
import bisect

from tests import membuf_ref as MB
from tests import memread_ref as MRD
from tests import mvcc_ref as R

NO_LIMIT = R.NO_LIMIT


class SnapshotIter:
    """the scanner over the store's keys of one range, in iteration order; stepping onto a locked key raises mvcc_ref.ErrLocked"""

    def __init__(self, store, keys, ts):
        self.store, self.keys, self.ts, self.i, self.valid = store, keys, ts, -1, True
        self.Next()

    def Next(self):
        while True:
            self.i += 1
            if self.i >= len(self.keys):
                self.valid = False
                return
            v = self.store.get_value(self.keys[self.i], self.ts)  # raises ErrLocked
            if v:
                self.key, self.value = self.keys[self.i], v
                return

    def Valid(self):
        return self.valid


class DirtyIter:
    """memDbBuffer.Iter / IterReverse over one range: the buffer's PUT and DEL entries (a DEL has an empty value); a lock-only key is
    not in the reference's buffer"""

    def __init__(self, pairs):
        self.pairs, self.i = pairs, 0

    def Valid(self):
        return self.i < len(self.pairs)

    def Next(self):
        self.i += 1

    @property
    def key(self):
        return self.pairs[self.i][0]

    @property
    def value(self):
        return self.pairs[self.i][1]


class UnionIter:
    """kv.UnionIter, line by line; dangling counts the "delete a record not exists?" warnings"""

    def __init__(self, dirty, snapshot, reverse):
        self.dirtyIt, self.snapshotIt, self.reverse = dirty, snapshot, reverse
        self.dirtyValid, self.snapshotValid = dirty.Valid(), snapshot.Valid()
        self.curIsDirty, self.isValid = False, False
        self.updateCur()

    def dirtyNext(self):
        self.dirtyIt.Next()
        self.dirtyValid = self.dirtyIt.Valid()

    def snapshotNext(self):
        self.snapshotIt.Next()
        self.snapshotValid = self.snapshotIt.Valid()

    def updateCur(self):
        self.isValid = True
        while True:
            if not self.dirtyValid and not self.snapshotValid:
                self.isValid = False
                break
            if not self.dirtyValid:
                self.curIsDirty = False
                break
            if not self.snapshotValid:
                self.curIsDirty = True
                if len(self.dirtyIt.value) == 0:
                    self.dirtyNext()
                    continue
                break
            sk, dk = self.snapshotIt.key, self.dirtyIt.key
            cmp = (dk > sk) - (dk < sk)
            if self.reverse:
                cmp = -cmp
            if cmp == 0:
                if len(self.dirtyIt.value) == 0:
                    self.dirtyNext()
                    self.snapshotNext()
                    continue
                self.snapshotNext()
                self.curIsDirty = True
                break
            elif cmp > 0:
                self.curIsDirty = False
                break
            else:
                if len(self.dirtyIt.value) == 0:
                    self.dirtyNext()
                    continue
                self.curIsDirty = True
                break

    def Next(self):
        if not self.curIsDirty:
            self.snapshotNext()
        else:
            self.dirtyNext()
        self.updateCur()

    def Valid(self):
        return self.isValid

    def Key(self):
        return self.dirtyIt.key if self.curIsDirty else self.snapshotIt.key

    def Value(self):
        return self.dirtyIt.value if self.curIsDirty else self.snapshotIt.value


class Dirty:
    """the buffer's PUT and DEL entries, ascending, computed once for the many reads of a test (pass it wherever a model goes)"""

    def __init__(self, model):
        self.entries = MRD.entries(model) if model is not None else []  # lock-only keys included: the device keeps them
        self.pairs = [(k, v) for op, k, v in self.entries if op in (MB.OP_PUT, MB.OP_DEL)]
        self.keys = [k for k, _ in self.pairs]
        self.all_keys = [k for _, k, _ in self.entries]

    @staticmethod
    def _cut(keys, start, end):
        lo = bisect.bisect_left(keys, start) if start else 0
        hi = bisect.bisect_left(keys, end) if end else len(keys)
        return lo, max(lo, hi)

    def in_range(self, start, end):
        lo, hi = self._cut(self.keys, start, end)
        return self.pairs[lo:hi]

    def entries_in_range(self, start, end):
        lo, hi = self._cut(self.all_keys, start, end)
        return self.entries[lo:hi]


def as_dirty(model):
    return model if isinstance(model, Dirty) else Dirty(model)


def dirty_entries(model):
    """[(key, value)] of the buffer's PUT and DEL entries, ascending (model None: lazyMemBuffer never written)"""
    return as_dirty(model).pairs


def open_iter(store, model, start, end, ts, desc):
    """BufferStore.Iter(start, end) / IterReverse over [start, end) (an empty start: from the first key, an empty end: to the last)"""
    if start and end and start >= end:
        keys, dirty = [], []
    else:
        keys = store._range(start, end)
        dirty = as_dirty(model).in_range(start, end)
    if desc:
        keys, dirty = keys[::-1], dirty[::-1]
    return UnionIter(DirtyIter(dirty), SnapshotIter(store, keys, ts), desc)


class Locked(Exception):
    """the lock error of a read, with the pairs taken before it"""

    def __init__(self, err, n_pairs):
        Exception.__init__(self, "key is locked")
        self.err, self.n_pairs = err, n_pairs

    def fields(self):
        return self.err.fields()


def read(store, model, ranges, ts, desc=False, limit=-1):
    """tsq_unionstore_scan: -> dict(pairs, from_buffer, range_counts); raises Locked"""
    left = NO_LIMIT if limit is None or limit < 0 else limit
    pairs, fb, counts = [], [], []
    for start, end in ranges:
        n = 0
        if len(pairs) < left:
            try:
                it = open_iter(store, model, start, end, ts, desc)
                while it.Valid():
                    pairs.append((it.Key(), it.Value()))
                    fb.append(1 if it.curIsDirty else 0)
                    n += 1
                    if len(pairs) >= left:
                        break
                    it.Next()
            except R.ErrLocked as e:
                raise Locked(e, len(pairs))
        counts.append(n)
    return dict(pairs=pairs, from_buffer=fb, range_counts=counts)


def visible(store, key, ts):
    try:
        return bool(store.get_value(key, ts))
    except R.ErrLocked:
        return False


def scan_stats(store, model, ranges, ts):
    """the counts of tsq_unionstore_result that do not depend on the limit: over every position the ranges examine"""
    d = as_dirty(model)
    ps = pb = shadowed = dels = dangling = 0
    for start, end in ranges:
        if start and end and start >= end:
            continue
        keys = store._range(start, end)
        ps += len(keys)
        for op, k, _ in d.entries_in_range(start, end):
            pb += 1
            vis = op != MB.OP_LOCK and visible(store, k, ts)
            if op == MB.OP_DEL:
                dels += 1
                dangling += not vis
            shadowed += vis
    return dict(positions_snapshot=ps, positions_buffer=pb, shadowed=shadowed, skipped_dels=dels, dangling_dels=dangling)


def get(store, model, keys, ts):
    """tsq_unionstore_get: BufferStore.Get of every key in input order -> [value or None]; the first key that meets a lock raises
    Locked (n_pairs = the values found before it).  A buffer DEL answers None without reading the snapshot."""
    held = dict(as_dirty(model).pairs)
    out = []
    for k in keys:
        if k in held:
            out.append(held[k] or None)
            continue
        try:
            out.append((store.get(k, ts) or None) if k else None)
        except R.ErrLocked as e:
            raise Locked(e, sum(v is not None for v in out))
    return out


def Iter(store, model, start, end, ts):
    it = open_iter(store, model, start, end, ts, False)
    while it.Valid():
        yield it.Key(), it.Value()
        it.Next()


def IterReverse(store, model, k, ts):
    it = open_iter(store, model, b"", k, ts, True)
    while it.Valid():
        yield it.Key(), it.Value()
        it.Next()
