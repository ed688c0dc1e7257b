"""Shared by the GPU tests of the MVCC range calls: one call — ScanLock, ResolveLock / BatchResolveLock, GC, DeleteRange or a write —
answered by the model (tests/mvcc_maint_ref.py) and by the GPU through tinysql_amd.mvcc: the call's own answer, whether a next store
came back, the counts, then the full export against the model's arrays and reads."""
from tests import mvcc_gpu_helpers as G
from tests import mvcc_maint_ref as MM
from tests import mvcc_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import mvcc_write_ref as W
from tinysql_amd import mvcc as M

WRITES = ("prewrite", "commit", "rollback")


def n_versions(s):
    return sum(len(v) for v in s.versions.values())


def check_reads(ms, s):
    for ts in WG.read_timestamps(s):
        G.check(ms, s, [(b"", b"")], ts)
    G.check(ms, s, [(b"", b"")], R.U64_MAX, True, 5)


def step(ms, s, call, reads=True):
    """one call on the GPU store ms and on the model s (updated in place).  Returns (the next store or None when the call changed
    nothing or was refused — ms stays open and is the caller's to close — and the model's answer)."""
    if call[0] in WRITES:
        return WG.step(ms, s, call, reads)
    before = W.clone(s)
    want = MM.apply_call(s, call)
    if call[0] == "scan_lock":
        got = ms.scan_lock(call[1], call[2], call[3])
        lock_keys = sorted(s.locks)
        assert [l.fields() for l in got] == want, call
        assert [l.Index for l in got] == [lock_keys.index(k) for _, _, k in want]
        assert ms.last_scan_lock["n_locks"] == len(want) and ms.last_scan_lock["key_bytes"] == sum(len(k) for _, _, k in want)
        return None, want
    if call[0] == "gc":
        try:
            nxt = ms.gc(call[1], call[2], call[3])
        except M.ErrGCLocked as e:
            assert want[0] == "locked" and (e.Key, e.StartTS, e.SafePoint) == (want[1][0], before.locks[want[1][0]].start_ts, call[3]), call
            lm = ms.last_maint
            assert lm["n_errors"] == len(want[1]) and lm["first_error"] == sorted(before.locks).index(want[1][0]) and lm["versions_removed"] == 0
            WG.compare_store(ms, before)  # nothing is written
            return None, want
        assert want[0] == "ok", call
        changed = want[1]
    else:
        nxt = ms.batch_resolve_lock(call[1], call[2], call[3]) if call[0] == "resolve" else ms.delete_range(call[1], call[2])
        changed = want
    lm = ms.last_maint
    assert (nxt is not ms) == changed, (call, lm)
    assert lm["n_errors"] == 0 and lm["first_error"] == -1
    if not changed:
        assert (lm["versions_added"], lm["versions_replaced"], lm["versions_removed"], lm["locks_removed"]) == (0, 0, 0, 0), call
        WG.compare_store(ms, s)
        return None, want
    WG.compare_store(nxt, s)
    assert nxt.n == n_versions(before) + lm["versions_added"] - lm["versions_replaced"] - lm["versions_removed"] == n_versions(s)
    assert nxt.n_locks == len(before.locks) - lm["locks_removed"] == len(s.locks)
    if reads:
        check_reads(nxt, s)
    return nxt, want


def run_calls(ctx, s, calls, reads=True):
    """a history from the model store s: every call on the newest store; the stores before it are closed.  Returns (the last store,
    the names of the calls that changed the store, the names of those that did not)"""
    ms, changed, unchanged = WG.open_rw(ctx, s), set(), set()
    for call in calls:
        call = call(s) if callable(call) else call
        nxt, _ = step(ms, s, call, reads)
        (changed if nxt is not None else unchanged).add(call[0])
        if nxt is not None:
            ms.close()
            ms = nxt
    return ms, changed, unchanged
