"""Shared by the GPU tests of the MVCC writes: a model store (tests/mvcc_ref.py) uploaded writable, and one write call answered by
the model (tests/mvcc_write_ref.py) and by the GPU through tinysql_amd.mvcc — the verdict of every key with its fields, then the
full export against the model's arrays, then reads."""
from tests import mvcc_gpu_helpers as G
from tests import mvcc_ref as R
from tests import mvcc_write_ref as W
from tinysql_amd import mvcc as M


def open_rw(ctx, s):
    return M.MvccStore.create_rw(ctx, W.flat_rw(s))


def error_verdict(e):
    """an entry of a write exception's .errors as the model's verdict, a lock by its fields"""
    if e is None:
        return None
    if isinstance(e, M.ErrLocked):
        return (W.LOCKED, (e.Key, e.Primary, e.StartTS, e.TTL, e.LockType))
    if isinstance(e, M.ErrConflict):
        return (W.CONFLICT, e.StartTS, e.ConflictTS, e.ConflictCommitTS, e.Key)
    if isinstance(e, M.ErrRetryable):
        return (W.TXN_NOT_FOUND, e.Message)
    assert isinstance(e, M.ErrAlreadyCommitted)
    return (W.ALREADY_COMMITTED, e.CommitTS)


def model_error(s, call, key, v):
    if v[0] < W.LOCKED:
        return None
    if v[0] == W.LOCKED:
        lk = sorted(s.locks)[v[1]]
        return (W.LOCKED, R.ErrLocked(lk, s.locks[lk]).fields())
    if v[0] == W.CONFLICT:
        return (W.CONFLICT, call[3], v[1], v[2], key)
    return (W.TXN_NOT_FOUND, "txn not found") if v[0] == W.TXN_NOT_FOUND else (W.ALREADY_COMMITTED, v[1])


def call_keys(call):
    return [m[1] for m in call[1]] if call[0] == "prewrite" else list(call[1])


def gpu_call(ms, call):
    """-> the next MvccStore; raises what the mirror raises"""
    if call[0] == "prewrite":
        return ms.prewrite(call[1], call[2], call[3], call[4])
    if call[0] == "commit":
        return ms.commit(call[1], call[2], call[3])
    return ms.rollback(call[1], call[2])


def compare_store(ms, s):
    got, want = ms.export(), W.flat_rw(s)
    assert sorted(got) == sorted(want)
    assert W.same_flat(want, got) is None, W.same_flat(want, got)


def read_timestamps(s):
    cts = sorted({v.commit_ts for vs in s.versions.values() for v in vs})
    pick = cts[:: max(1, len(cts) // 3)][:3]
    return sorted({0, R.U64_MAX, R.U64_MAX - 1} | set(pick) | {max(c - 1, 0) for c in pick})


def step(ms, s, call, reads=True):
    """one write call on the GPU store ms and on the model s (which is updated in place when the call applies).  Returns (the next
    store — ms itself stays open and is the caller's to close — or None after errors, the model's verdicts)."""
    before = W.clone(s)
    verdicts, applied = W.apply_call(s, call)
    keys = call_keys(call)
    try:
        nxt = gpu_call(ms, call)
    except (M.ErrLocked, M.WriteError) as e:
        assert not applied, (call, verdicts)
        want = [model_error(before, call, k, v) for k, v in zip(keys, verdicts)]
        assert [error_verdict(x) for x in e.errors] == want, call
        assert error_verdict(e) == want[W.first_error(verdicts, keys)], call
        compare_store(ms, before)  # any error writes nothing
        return None, verdicts
    assert applied, (call, verdicts)
    compare_store(nxt, s)
    lw = nxt.last_write
    n_before = sum(len(v) for v in before.versions.values())
    assert lw["n_errors"] == 0 and lw["first_error"] == -1 and nxt.n == n_before + lw["versions_added"] - lw["versions_replaced"]
    assert nxt.n_locks == len(before.locks) + lw["locks_added"] - lw["locks_removed"] == len(s.locks)
    if reads:
        for ts in read_timestamps(s):
            G.check(nxt, s, [(b"", b"")], ts)
        G.check(nxt, s, [(b"", b"")], R.U64_MAX, True, 5)
    return nxt, verdicts


def run_calls(ctx, s, calls, reads=True):
    """a history from the model store s: every call on the newest store; the stores before it are closed.  Returns (the last store,
    the kinds met)"""
    ms, kinds = open_rw(ctx, s), set()
    for call in calls:
        call = call(s) if callable(call) else call
        nxt, verdicts = step(ms, s, call, reads)
        kinds |= W.call_kinds(call, verdicts)
        if nxt is not None:
            ms.close()
            ms = nxt
    return ms, kinds
