"""The reference's range calls (store/mockstore/mocktikv/mvcc_leveldb.go: ScanLock :906-939, ResolveLock :942-978, BatchResolveLock
:981-1019, GC :1022-1085, DeleteRange :1088-1090) stated over tests/mvcc_ref.Store, with what tsq_mvcc_resolve_lock / gc /
delete_range add to them: whether the call changed anything (a call that did not returns no next store).
tests/golden/mvcc_maint_cases.json holds this model to the reference's own tests; the host build of tsq_mvcc_maint_dp.h and the GPU
are held to this model."""
import bisect

import numpy as np

from tests import mvcc_ref as R
from tests import mvcc_write_ref as W


def in_range(keys, start, end):
    """newScanIterator (:149-171) over sorted keys: an empty start is the first key, an empty end the last, start >= end nothing"""
    lo = bisect.bisect_left(keys, start) if start else 0
    hi = bisect.bisect_left(keys, end) if end else len(keys)
    return keys[lo:hi]


def scan_lock(s, start, end, max_ts):
    """-> [(primary, start_ts, key)] in key order: LockInfo{PrimaryLock, LockVersion, Key} (:923-928)"""
    return [(s.locks[k].primary, s.locks[k].start_ts, k) for k in in_range(sorted(s.locks), start, end) if s.locks[k].start_ts <= max_ts]


def batch_resolve_lock(s, start, end, txn_infos):
    """txn_infos: {start_ts: commit_ts}.  -> changed.  commitLock (:590-613) / rollbackLock (:686-700) per matching lock"""
    changed = False
    for key in in_range(sorted(s.locks), start, end):
        lock = s.locks[key]
        if lock.start_ts not in txn_infos:
            continue
        commit_ts = txn_infos[lock.start_ts]
        if commit_ts > 0:
            if lock.op != R.OP_LOCK:
                s._insert(key, R.Value(R.PUT if lock.op == R.OP_PUT else R.DELETE, lock.start_ts, commit_ts, lock.value))
        else:
            s._insert(key, R.Value(R.ROLLBACK, lock.start_ts, lock.start_ts, b""))
        del s.locks[key]
        changed = True
    return changed


def resolve_lock(s, start, end, start_ts, commit_ts):
    return batch_resolve_lock(s, start, end, {start_ts: commit_ts})


def gc_locks(s, start, end, safe_point):
    """the locks that refuse a GC (:1041-1047), in key order"""
    return [k for k in in_range(sorted(s.locks), start, end) if s.locks[k].start_ts <= safe_point]


def gc(s, start, end, safe_point):
    """-> ("locked", [keys]) and nothing written, or ("ok", changed) (:1049-1080)"""
    bad = gc_locks(s, start, end, safe_point)
    if bad:
        return "locked", bad
    changed = False
    for key in in_range(sorted(s.versions), start, end):
        keep_next, out = True, []
        for v in s.versions[key]:
            if v.commit_ts > safe_point:
                out.append(v)
                continue
            if v.type in (R.PUT, R.DELETE):
                if keep_next and v.type == R.PUT:
                    out.append(v)
                keep_next = False
        if len(out) != len(s.versions[key]):
            changed = True
            if out:
                s.versions[key] = out
            else:
                del s.versions[key]
    return "ok", changed


def delete_range(s, start, end):
    """-> changed.  The bounds are EncodeBytes(start) and EncodeBytes(end) over the raw LevelDB keys mvccEncode(key, ver) (:1088-1090,
    :1231-1246) — stated here in exactly that encoded form, so that the empty end's meaning comes from the encoding, not from a rule"""
    lo, hi = R.encode_bytes(start), R.encode_bytes(end)
    changed = False
    for key in list(s.versions):
        keep = [v for v in s.versions[key] if not (lo <= R.mvcc_encode(key, v.commit_ts) < hi)]
        if len(keep) != len(s.versions[key]):
            changed = True
            if keep:
                s.versions[key] = keep
            else:
                del s.versions[key]
    for key in list(s.locks):
        if lo <= R.mvcc_encode(key, R.LOCK_VER) < hi:
            del s.locks[key]
            changed = True
    return changed


# ---------------------------------------------------------------------- calls as tuples (shared by the CPU and the GPU tests)
def apply_call(s, call):
    """("scan_lock", start, end, max_ts) -> the list; ("resolve", start, end, {start_ts: commit_ts}) -> changed; ("gc", start, end,
    safe_point) -> ("locked", keys) | ("ok", changed); ("delete_range", start, end) -> changed; a write call of mvcc_write_ref ->
    (verdicts, applied)"""
    if call[0] == "scan_lock":
        return scan_lock(s, call[1], call[2], call[3])
    if call[0] == "resolve":
        return batch_resolve_lock(s, call[1], call[2], call[3])
    if call[0] == "gc":
        return gc(s, call[1], call[2], call[3])
    if call[0] == "delete_range":
        return delete_range(s, call[1], call[2])
    return W.apply_call(s, call)


def random_bound(s, rng):
    ks = s.keys() or [b"m"]
    k = ks[int(rng.integers(0, len(ks)))]
    w = rng.random()
    if w < 0.35:
        return k
    if w < 0.5:
        return k + b"\x00"
    if w < 0.6:
        return k[:-1] if len(k) > 1 else k
    if w < 0.7:
        return b"\x00" if rng.random() < 0.5 else b"\xff\xff"
    return b""


def random_range(s, rng):
    a, b = random_bound(s, rng), random_bound(s, rng)
    if a and b and a > b and rng.random() < 0.8:
        a, b = b, a
    return a, b


def random_maint_call(s, rng):
    """one of the four range calls with a range and timestamps around the store's own"""
    start, end = random_range(s, rng)
    lts = sorted({l.start_ts for l in s.locks.values()})
    cts = sorted({v.commit_ts for vs in s.versions.values() for v in vs})
    w = rng.random()
    if w < 0.25:
        ts = lts[int(rng.integers(0, len(lts)))] + int(rng.integers(-1, 2)) if lts and rng.random() < 0.8 else R.U64_MAX
        return ("scan_lock", start, end, min(max(ts, 0), R.U64_MAX))
    if w < 0.55:
        infos = {}
        for _ in range(int(rng.integers(0, 4))):
            st = lts[int(rng.integers(0, len(lts)))] if lts and rng.random() < 0.8 else int(rng.integers(0, 2000))
            if rng.random() < 0.4:
                infos[st] = 0 if st < R.U64_MAX else 1
            elif rng.random() < 0.2 and cts:
                infos[st] = max(1, min(cts[int(rng.integers(0, len(cts)))], R.U64_MAX - 1))  # an existing commitTS: may replace
            else:
                infos[st] = min(st + int(rng.integers(1, 5)), R.U64_MAX - 1)
        return ("resolve", start, end, infos)
    if w < 0.85:
        sp = cts[int(rng.integers(0, len(cts)))] + int(rng.integers(-1, 2)) if cts and rng.random() < 0.85 else int(rng.integers(0, 100))
        return ("gc", start, end, min(max(sp, 0), R.U64_MAX))
    if rng.random() < 0.5:  # a narrow range: a history that deletes everything early checks little
        ks = s.keys() or [b"m"]
        i = int(rng.integers(0, len(ks)))
        start, end = ks[i], ks[min(i + int(rng.integers(0, 4)), len(ks) - 1)]
    return ("delete_range", start, end)


def random_call(s, rng, txns, fresh_keys, maint_share=0.5):
    """a history step: a range call, or a write call of mvcc_write_ref.random_call"""
    if rng.random() < maint_share:
        return random_maint_call(s, rng)
    return W.random_call(s, rng, txns, fresh_keys)
