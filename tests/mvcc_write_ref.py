"""The reference's two-phase-commit writes (store/mockstore/mocktikv/mvcc_leveldb.go: Prewrite :442-537, Commit :540-613, Rollback
:616-700, getTxnCommitInfo :702-717) stated over tests/mvcc_ref.Store, with what tsq_mvcc_prewrite / commit / rollback add to them:
every key gets a verdict, any error writes nothing, first_error is the reference's error.  tests/golden/mvcc_write_cases.json holds
this model to the reference's own tests; the host build of tsq_mvcc_write_dp.h and the GPU are held to this model.
A verdict is (code, info0, info1): LOCKED carries the lock's index among the store's sorted lock keys, CONFLICT ConflictTS and
ConflictCommitTS, ALREADY_COMMITTED the commitTS."""
import numpy as np

from tests import mvcc_ref as R

OK, NOOP, LOCKED, CONFLICT, TXN_NOT_FOUND, ALREADY_COMMITTED = 0, 1, 2, 3, 4, 5
NAMES = {"ok": OK, "noop": NOOP, "locked": LOCKED, "conflict": CONFLICT, "txn_not_found": TXN_NOT_FOUND, "already_committed": ALREADY_COMMITTED}


def lock_index(s, key):
    return sorted(s.locks).index(key)


def txn_version(s, key, start_ts):
    """getTxnCommitInfo: the first version of the chain with start_ts == startTS"""
    for v in s.versions.get(key, []):
        if v.start_ts == start_ts:
            return v
    return None


def prewrite_verdict(s, key, start_ts):
    lock = s.locks.get(key)
    if lock is not None:
        return (LOCKED, lock_index(s, key), 0) if lock.start_ts != start_ts else (OK, 0, 0)
    vs = s.versions.get(key, [])
    commit_ts, vstart = (vs[0].commit_ts, vs[0].start_ts) if vs else (0, 0)
    return (CONFLICT, vstart, commit_ts) if commit_ts >= start_ts else (OK, 0, 0)


def commit_verdict(s, key, start_ts):
    lock = s.locks.get(key)
    if lock is not None and lock.start_ts == start_ts:
        return (OK, 0, 0)
    c = txn_version(s, key, start_ts)
    return (NOOP, 0, 0) if c is not None and c.type != R.ROLLBACK else (TXN_NOT_FOUND, 0, 0)


def rollback_verdict(s, key, start_ts):
    lock = s.locks.get(key)
    if lock is not None and lock.start_ts == start_ts:
        return (OK, 0, 0)
    c = txn_version(s, key, start_ts)
    if c is None:
        return (OK, 0, 0)
    return (ALREADY_COMMITTED, c.commit_ts, 0) if c.type != R.ROLLBACK else (NOOP, 0, 0)


def first_error(verdicts, keys):
    """the index (in `keys`' order) of the error the reference would return: Prewrite's list is per mutation; Commit and Rollback
    stop at the first failing key of the request, which the committer hands over in key order"""
    bad = [i for i, v in enumerate(verdicts) if v[0] >= LOCKED]
    return min(bad, key=lambda i: keys[i]) if bad else -1


def prewrite(s, mutations, primary, start_ts, ttl=0):
    """-> (verdicts per mutation, applied).  Each verdict reads the store, not the other mutations of the request (:497)."""
    verdicts = [prewrite_verdict(s, key, start_ts) for _, key, _ in mutations]
    if any(v[0] >= LOCKED for v in verdicts):
        return verdicts, False
    for op, key, value in mutations:  # (a key named twice: the later batch.Put wins)
        s.locks[key] = R.Lock(start_ts, primary, value, op, ttl)
    return verdicts, True


def commit(s, keys, start_ts, commit_ts):
    assert len(set(keys)) == len(keys)
    verdicts = [commit_verdict(s, key, start_ts) for key in keys]
    if any(v[0] >= LOCKED for v in verdicts):
        return verdicts, False
    for key, v in zip(keys, verdicts):
        if v[0] == OK:
            lock = s.locks.pop(key)
            if lock.op != R.OP_LOCK:
                s._insert(key, R.Value(R.PUT if lock.op == R.OP_PUT else R.DELETE, start_ts, commit_ts, lock.value))
    return verdicts, True


def rollback(s, keys, start_ts):
    assert len(set(keys)) == len(keys)
    verdicts = [rollback_verdict(s, key, start_ts) for key in keys]
    if any(v[0] >= LOCKED for v in verdicts):
        return verdicts, False
    for key, v in zip(keys, verdicts):
        if v[0] == OK:
            lock = s.locks.get(key)
            if lock is not None and lock.start_ts == start_ts:
                del s.locks[key]
            s._insert(key, R.Value(R.ROLLBACK, start_ts, start_ts, b""))
    return verdicts, True


def flat_rw(s):
    """Store.flat() plus the locks' values: what MvccStore.create_rw takes and MvccStore.export returns"""
    f = s.flat()
    vals = [s.locks[k].value for k in sorted(s.locks)]
    offs = np.zeros(len(vals) + 1, dtype=np.int64)
    if vals:
        offs[1:] = np.cumsum([len(v) for v in vals])
    f["lock_values"], f["lock_value_offsets"] = np.frombuffer(b"".join(vals), dtype=np.uint8).copy(), offs
    return f


def same_flat(a, b):
    """None, or the name of the first array that differs"""
    for name in a:
        x, y = np.asarray(a[name]), np.asarray(b[name])
        if x.shape != y.shape or not np.array_equal(x, y):
            return name
    return None


def clone(s):
    c = R.Store()
    c.versions = {k: list(v) for k, v in s.versions.items()}
    c.locks = dict(s.locks)
    return c


def writable_random_store(rng, n_keys, style="prefix", max_chain=5):
    """mvcc_ref.random_store with what a writable store must satisfy: no put lock with an empty value (its locks carry b"x" / b"y"),
    lock ops the reference can have written (Put / Del / Lock)"""
    s = R.random_store(rng, n_keys, style, max_chain=max_chain) if n_keys else R.Store()
    for k, l in list(s.locks.items()):
        if l.op == R.OP_ROLLBACK:
            s.locks[k] = l._replace(op=R.OP_DEL)
    return s


# ---------------------------------------------------------------------- random histories (shared by the CPU and the GPU tests)
def random_call(s, rng, txns, fresh_keys):
    """one write call of one of the interleaved transactions `txns` (start timestamps): ("prewrite", mutations, primary, start_ts,
    ttl) | ("commit", keys, start_ts, commit_ts) | ("rollback", keys, start_ts).  Keys come from the store's keys, its locks, and
    fresh ones; timestamps sit around the store's own, so that every verdict kind is met."""
    pool = s.keys() + list(fresh_keys)
    if not pool:
        pool = [b"k0"]
    m = int(rng.integers(1, 6))
    keys = sorted({pool[int(rng.integers(0, len(pool)))] for _ in range(m)})
    w = rng.random()
    ts = txns[int(rng.integers(0, len(txns)))]
    if w < 0.2:  # a timestamp of a version or a lock of one of the keys: conflicts, already-committed, the own lock
        k = keys[0]
        cand = [v.start_ts for v in s.versions.get(k, [])] + ([s.locks[k].start_ts] if k in s.locks else [])
        if cand:
            ts = cand[int(rng.integers(0, len(cand)))]
    kind = rng.random()
    if kind < 0.4:
        muts = []
        for k in keys:
            op = int(rng.choice([R.OP_PUT, R.OP_PUT, R.OP_DEL, R.OP_LOCK]))
            muts.append((op, k, b"w%d-" % ts + bytes(rng.integers(97, 123, int(rng.integers(0, 9)), dtype=np.uint8)) if op == R.OP_PUT else b""))
        return ("prewrite", muts, keys[0], ts, int(rng.integers(0, 100)))
    if kind < 0.75:
        cts = min(R.U64_MAX - 1, ts + int(rng.integers(0, 4)))
        if rng.random() < 0.15:
            vs = s.versions.get(keys[0], [])
            if vs:
                cts = vs[int(rng.integers(0, len(vs)))].commit_ts  # an existing (key, commitTS): replaced
        return ("commit", keys, ts, cts)
    return ("rollback", keys, min(ts, R.U64_MAX - 1))


def apply_call(s, call):
    """-> (verdicts, applied) of the model"""
    if call[0] == "prewrite":
        return prewrite(s, call[1], call[2], call[3], call[4])
    if call[0] == "commit":
        return commit(s, call[1], call[2], call[3])
    return rollback(s, call[1], call[2])


def call_kinds(call, verdicts):
    """the names the random-history tests count: every error kind and the two no-ops"""
    out = set()
    for v in verdicts:
        if v[0] == NOOP:
            out.add("noop_" + call[0])
        elif v[0] >= LOCKED:
            out.add({LOCKED: "locked", CONFLICT: "conflict", TXN_NOT_FOUND: "txn_not_found", ALREADY_COMMITTED: "already_committed"}[v[0]])
    return out


ALL_KINDS = {"locked", "conflict", "txn_not_found", "already_committed", "noop_commit", "noop_rollback"}


def scripted_calls(a, b, c):
    """nine calls of two transactions (startTS 30 and 35) over three keys the store does not hold (a < b < c), which meet every
    error kind and both no-ops once, whatever else the store holds; the random calls of a history follow them"""
    return [("prewrite", [(R.OP_PUT, a, b"a30"), (R.OP_PUT, b, b"b30")], a, 30, 7),
            ("prewrite", [(R.OP_PUT, b, b"b35"), (R.OP_PUT, c, b"c35")], b, 35, 0),  # locked by 30 on b
            ("commit", [a], 30, 40),
            ("commit", [a], 30, 40),  # committed already: no-op
            ("prewrite", [(R.OP_DEL, a, b"")], a, 35, 0),  # commitTS 40 >= 35: conflict
            ("rollback", [a], 30),  # already committed at 40
            ("rollback", [b], 30),
            ("rollback", [b], 30),  # rolled back already: no-op
            ("commit", [b], 30, 41)]  # txn not found
