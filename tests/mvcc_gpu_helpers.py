"""Shared by the GPU tests of tsq_mvcc_*: a model store (tests/mvcc_ref.py) uploaded through tinysql_amd.mvcc, and one read answered
by both — pairs, per-range counts and the lock's fields are compared exactly."""
from tests import mvcc_ref as R
from tinysql_amd import mvcc as M


def open_store(ctx, s):
    s.freeze()
    return M.MvccStore(ctx, s.flat())


def gpu_answer(ms, ranges, ts, desc=False, limit=None):
    try:
        p = ms.scan(ranges, ts, desc, limit)
    except M.ErrLocked as e:
        return ("locked", (e.Key, e.Primary, e.StartTS, e.TTL, e.LockType))
    try:
        return ("ok", p.to_host(), p.counts)
    finally:
        p.free()


def model_answer(s, ranges, ts, desc=False, limit=None):
    try:
        pairs, counts = R.read_ranges(s, ranges, ts, desc, limit)
        return ("ok", pairs, counts)
    except R.ErrLocked as e:
        return ("locked", e.fields())


def check(ms, s, ranges, ts, desc=False, limit=None):
    """the ranges as the caller of tsq_mvcc_scan hands them in (already reversed for desc); returns the model's answer"""
    want = model_answer(s, ranges, ts, desc, limit)
    got = gpu_answer(ms, ranges, ts, desc, limit)
    assert got == want, (ranges[:4], ts, desc, limit, got[0], want[0], got[1:][:1] if got[0] == "locked" else len(got[1]))
    return want
