"""The reference's transaction buffer stated as a dict: kv.memDbBuffer (kv/memdb_buffer.go: Set :95-108, Delete :111-114, Get :86-92,
Size / Len :117-124) and the walk of twoPhaseCommitter.initKeysAndMutations over it (store/tikv/2pc.go:115-172) with primary()
(:211-216).  tests/golden/membuf_cases.json holds this model to the reference's own tests; the host build of tsq_membuf_dp.h and
the GPU (tsq_membuf_*) are held to this model.

Two places follow the reference's SEQUENTIAL semantics, which tsq_membuf_* departs from on purpose (include/tsq.h, the two pinned
departures): a Set that fails has already let the earlier Sets in, and the total size is checked after every Set.  `Model.finish`
states what tsq_membuf_finish answers instead: one check of the final size."""

SET, DELETE, LOCK = 0, 1, 2
OP_PUT, OP_DEL, OP_LOCK = 0, 1, 2


class ErrCannotSetNilValue(Exception):
    pass


class ErrEntryTooLarge(Exception):
    pass


class ErrTxnTooLarge(Exception):
    pass


class ErrNotExist(Exception):
    pass


class Model:
    def __init__(self, entry_size_limit=0, total_size_limit=0):
        self.entry_size_limit, self.total_size_limit = entry_size_limit, total_size_limit
        self.db = {}          # key -> value; b"" = deleted
        self.lock_keys = []   # tikvTxn.lockKeys, in push order, duplicates kept

    # ------------------------------------------------------------------ memDbBuffer
    def Size(self):
        return sum(len(k) + len(v) for k, v in self.db.items())

    def Len(self):
        return len(self.db)

    def Set(self, k, v):
        if len(v) == 0:
            raise ErrCannotSetNilValue()
        if self.entry_size_limit and len(k) + len(v) > self.entry_size_limit:
            raise ErrEntryTooLarge(self.entry_size_limit, len(k) + len(v))
        self.db[bytes(k)] = bytes(v)
        if self.total_size_limit and self.Size() > self.total_size_limit:
            raise ErrTxnTooLarge(self.Size())

    def Delete(self, k):
        self.db[bytes(k)] = b""

    def LockKeys(self, *keys):
        self.lock_keys += [bytes(k) for k in keys]

    def Get(self, k):
        if k not in self.db:
            raise ErrNotExist()
        return self.db[k]

    def walk(self):
        """the sorted walk (WalkBuffer / the iterator from nil): [(key, value)] in bytes.Compare order"""
        return sorted(self.db.items())

    def push(self, kind, keys, values=None):
        """one tsq_membuf_push of the model, row by row (no checks beyond Set's)"""
        for i, k in enumerate(keys):
            if kind == SET:
                self.Set(k, values[i])
            elif kind == DELETE:
                self.Delete(k)
            else:
                self.LockKeys(k)

    # ------------------------------------------------------------------ initKeysAndMutations
    def mutations(self):
        """-> dict(entries=[(op, key, value)] in key order, puts, dels, locks, size, primary (the key c.keys[0], None when empty))"""
        muts, keys, size, puts, dels, locks = {}, [], 0, 0, 0, 0
        for k, v in self.walk():
            if v:
                muts[k] = (OP_PUT, k, v)
                puts += 1
            else:
                muts[k] = (OP_DEL, k, b"")
                dels += 1
            keys.append(k)
            size += len(k) + len(v)
        for k in self.lock_keys:
            if k not in muts:
                muts[k] = (OP_LOCK, k, b"")
                locks += 1
                keys.append(k)
                size += len(k)
        return dict(entries=[muts[k] for k in sorted(muts)], puts=puts, dels=dels, locks=locks, size=size, primary=keys[0] if keys else None)

    def finish(self):
        """what tsq_membuf_finish reports: mutations() with primary as an index into the entries (-1: empty); raises ErrTxnTooLarge on the
        FINAL size (the pinned departure)"""
        m = self.mutations()
        if self.total_size_limit and m["size"] > self.total_size_limit:
            raise ErrTxnTooLarge(m["size"])
        m["primary_index"] = [e[1] for e in m["entries"]].index(m["primary"]) if m["entries"] else -1
        return m


def replay(pushes, **limits):
    """[(kind, keys, values or None)] -> the Model after them"""
    m = Model(**limits)
    for kind, keys, values in pushes:
        m.push(kind, keys, values)
    return m


def first_refused_row(kind, keys, values, entry_size_limit=0):
    """the row tsq_membuf_push names in *error_row: the first empty key, nil value or too-large entry; -1: none"""
    for i, k in enumerate(keys):
        if len(k) == 0:
            return i
        if kind == SET and (len(values[i]) == 0 or (entry_size_limit and len(k) + len(values[i]) > entry_size_limit)):
            return i
    return -1
