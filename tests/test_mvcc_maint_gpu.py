"""GPU parity of the MVCC range calls (tsq_mvcc_scan_lock / scan_lock_fetch / resolve_lock / gc / delete_range) with the sequential
model of tests/mvcc_maint_ref.py: after every call its own answer, whether a next store came back, the full export against the model's
arrays, then reads against mvcc_ref.read_ranges."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import mvcc_gpu_helpers as G
from tests import mvcc_maint_gpu_helpers as MG
from tests import mvcc_maint_ref as MM
from tests import mvcc_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import mvcc_write_ref as W
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import mvcc as M

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = lambda s: s.encode("latin-1")
U64 = R.U64_MAX
PUT, DEL, LOCK = R.OP_PUT, R.OP_DEL, R.OP_LOCK
V = R.Value


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "mvcc_maint_cases.json")))["cases"]


def step_call(st):
    if st["op"] == "prewrite":
        return ("prewrite", [(R.OP_NAMES[m[0]], L1(m[1]), L1(m[2])) for m in st["mutations"]], L1(st["primary"]), st["start_ts"], st["ttl"])
    if st["op"] == "commit":
        return ("commit", [L1(k) for k in st["keys"]], st["start_ts"], st["commit_ts"])
    if st["op"] == "scan_lock":
        return ("scan_lock", L1(st["start"]), L1(st["end"]), st["max_ts"])
    if st["op"] == "resolve":
        return ("resolve", L1(st["start"]), L1(st["end"]), {int(a): int(b) for a, b in st["txns"]})
    if st["op"] == "gc":
        return ("gc", L1(st["start"]), L1(st["end"]), st["safe_point"])
    return ("delete_range", L1(st["start"]), L1(st["end"]))


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_the_references_steps(ctx, case):
    s = R.Store()
    ms = WG.open_rw(ctx, s)
    try:
        for st in case["steps"]:
            if st["op"] == "get":
                got = G.check(ms, s, [(L1(st["key"]), None)], st["ts"])
                assert got == ("ok", [] if st["expect"] is None else [(L1(st["key"]), L1(st["expect"]))], [0 if st["expect"] is None else 1]), st["line"]
                continue
            if st["op"] == "scan":
                got = G.check(ms, s, [(L1(st["start"]), L1(st["end"]))], st["ts"], False, st["limit"])
                assert got[0] == "ok" and got[1] == [(L1(k), L1(v)) for k, v in st["expect"]], st["line"]
                continue
            nxt, want = MG.step(ms, s, step_call(st))
            if st["op"] == "scan_lock":
                assert want == [(L1(l["primary"]), l["start_ts"], L1(l["key"])) for l in st["expect"]], st["line"]
            if nxt is not None:
                ms.close()
                ms = nxt
    finally:
        ms.close()


# ---------------------------------------------------------------- random histories
def gc_between_locks(s):
    """a GC over the first window of up to 8 neighbouring keys that no lock refuses and that drops something (random locks sit at
    low timestamps: a GC over everything is mostly refused)"""
    ks = s.keys()
    for i in range(len(ks)):
        call = ("gc", ks[i], ks[min(i + 8, len(ks) - 1)], U64)
        if MM.gc(W.clone(s), *call[1:]) == ("ok", True):
            return call
    return ("gc", b"", b"", 0)


@pytest.mark.parametrize("style", ["prefix", "record"])
@pytest.mark.parametrize("n_keys", [0, 1, 63, 64, 65, 2047, 2048, 2049])
def test_random_histories(ctx, n_keys, style):
    rng = np.random.default_rng(3000 + n_keys + (7 if style == "record" else 0))
    s = W.writable_random_store(rng, n_keys, style)
    fresh = [b"\x01first", b"Bmid", b"zz-last", b"\x01first\x00", b"Bmie"]
    txns = [30, 35, 1001, (1 << 63) + 5]
    big = n_keys > 1000
    # a prewrite the range calls can meet whatever the store holds, then the interleaved history
    calls = [("prewrite", [(PUT, fresh[0], b"f30"), (DEL, fresh[1], b""), (LOCK, fresh[2], b"")], fresh[0], 30, 7),
             ("scan_lock", b"", b"", U64), ("resolve", b"", b"C", {30: 40}), ("gc", b"", b"", 20), gc_between_locks, ("delete_range", fresh[2], fresh[2] + b"\x00")]
    calls += [lambda st: MM.random_call(st, rng, txns, fresh)] * (14 if big else 30)
    ms, changed, unchanged = MG.run_calls(ctx, s, calls, reads=not big)
    try:
        assert {"resolve", "delete_range"} <= changed and "scan_lock" in unchanged
        if n_keys >= 63:
            assert "gc" in changed
        G.check(ms, s, [(b"", b"")], U64 - 1)
        for r in R.random_ranges(s, rng, 4):
            G.check(ms, s, [r], 1001)
    finally:
        ms.close()


def run(ctx, s, calls):
    """the calls on a copy of s; returns the model after them (the stores are closed)"""
    t = W.clone(s)
    ms, _, _ = MG.run_calls(ctx, t, calls)
    ms.close()
    return t


# ---------------------------------------------------------------- GC edges
def test_gc_at_the_safe_point_and_one_above_and_at_2_63(ctx):
    for base in (100, (1 << 63) - 1, 1 << 63, U64 - 9):
        s = R.Store()
        s.versions[b"k"] = [V(PUT, base + 1, base + 2, b"c"), V(PUT, base - 1, base, b"b"), V(PUT, base - 3, base - 2, b"a")]
        s.versions[b"m"] = [V(PUT, base, base + 1, b"only")]
        t = run(ctx, s, [("gc", b"", b"", base - 1)])  # commit_ts == safe_point + 1: untouched; base - 2 is the only one under it and stays
        assert t.versions == s.versions
        t = run(ctx, s, [("gc", b"", b"", base)])  # commit_ts == safe_point: subject to GC — it is the keeper, the older one goes
        assert [v.value for v in t.versions[b"k"]] == [b"c", b"b"] and t.versions[b"m"] == s.versions[b"m"]
        t = run(ctx, s, [("gc", b"", b"", base + 2), ("gc", b"", b"", U64)])
        assert [v.value for v in t.versions[b"k"]] == [b"c"]


def test_gc_newest_under_the_safe_point_is_a_delete(ctx):
    s = R.Store()
    s.versions[b"gone"] = [V(DEL, 7, 8, b""), V(PUT, 3, 4, b"x")]  # nothing else: the key leaves the universe
    s.versions[b"newer"] = [V(PUT, 30, 31, b"n"), V(DEL, 7, 8, b""), V(PUT, 3, 4, b"x")]
    s.versions[b"locked"] = [V(DEL, 7, 8, b""), V(PUT, 3, 4, b"x")]
    s.locks[b"locked"] = R.Lock(25, b"locked", b"lv", PUT, 0)
    t = run(ctx, s, [("gc", b"", b"", 20)])
    assert sorted(t.versions) == [b"newer"] and t.keys() == [b"locked", b"newer"] and [v.value for v in t.versions[b"newer"]] == [b"n"]
    t = run(ctx, s, [("gc", b"gone", b"gone\x00", 20), ("scan_lock", b"", b"", U64), ("gc", b"", b"", 20), ("gc", b"", b"", 20)])
    assert t.keys() == [b"locked", b"newer"]


def test_gc_rollbacks_around_the_keeper_and_a_key_of_rollbacks_only(ctx):
    s = R.Store()
    RB = lambda c: V(R.ROLLBACK, c, c, b"")
    s.versions[b"a"] = [RB(19), RB(18), V(PUT, 16, 17, b"keep"), RB(15), V(PUT, 13, 14, b"old"), RB(12), V(DEL, 10, 11, b""), RB(9)]
    s.versions[b"r"] = [RB(5), RB(4), RB(3)]
    s.versions[b"top"] = [V(PUT, 40, 41, b"t"), RB(19), V(DEL, 17, 18, b""), RB(3)]
    t = run(ctx, s, [("gc", b"", b"", 20)])
    assert t.versions == {b"a": [V(PUT, 16, 17, b"keep")], b"top": [V(PUT, 40, 41, b"t")]}
    t = run(ctx, s, [("gc", b"", b"", 15)])  # the ROLLBACK at 15 in front of the keeper at 14
    assert [v.commit_ts for v in t.versions[b"a"]] == [19, 18, 17, 14] and b"r" not in t.versions


def chain_store(n, keeper):
    """as tests/test_mvcc_maint_cpu.chain_store: a key of n entries under the safe point 10 n + 5 and one above"""
    s = R.Store()
    vs = []
    for i in range(n):
        c = 10 * (n - i)
        t = R.ROLLBACK
        if keeper == "alternating":
            t = PUT if i % 2 == 0 else R.ROLLBACK
        elif (keeper == "first" and i == 0) or (keeper == "last" and i == n - 1):
            t = PUT
        vs.append(V(t, c - 1, c, b"p%d" % i if t == PUT else b""))
    s.versions[b"hot"] = [V(PUT, 10 * n + 8, 10 * n + 9, b"above")] + vs
    s.versions[b"a"] = [V(PUT, 1, 2, b"a")]
    s.versions[b"z"] = [V(DEL, 3, 4, b""), V(PUT, 1, 2, b"z")]
    return s


@pytest.mark.parametrize("wave_chain", [4, 64])
@pytest.mark.parametrize("n", [63, 64, 65, 300, 4097])
def test_gc_long_chains(ctx, n, wave_chain):
    ctx.set_knob(abi.KNOB_MVCC_WAVE_CHAIN, wave_chain)
    for keeper in ("first", "last", "absent", "alternating"):
        s = chain_store(n, keeper)
        ms = WG.open_rw(ctx, s)
        try:
            nxt, _ = MG.step(ms, s, ("gc", b"", b"", 10 * n + 5), reads=False)
            kept = [v.value for v in s.versions[b"hot"]]
            assert kept == ([b"above"] if keeper == "absent" else [b"above", b"p%d" % (n - 1 if keeper == "last" else 0)])
            assert nxt.get(b"hot", 10 * n + 5) == (kept[1] if len(kept) > 1 else None) and nxt.get(b"z", 50) is None and nxt.get(b"a", 50) == b"a"
            nx2, _ = MG.step(nxt, s, ("gc", b"", b"", 10 * n + 5), reads=False)
            assert nx2 is None
            nxt.close()
        finally:
            ms.close()


def test_gc_lock_refusal(ctx):
    s = R.Store()
    for k in (b"a", b"b", b"c", b"d"):
        s.versions[k] = [V(PUT, 3, 4, b"new"), V(PUT, 1, 2, b"old")]
    s.locks[b"a"] = R.Lock(5, b"a", b"v", PUT, 0)  # a low lock outside the range
    s.locks[b"c"] = R.Lock(50, b"c", b"v", PUT, 3)
    s.locks[b"d"] = R.Lock(40, b"c", b"v", PUT, 3)  # the later lock has the smaller timestamp
    ms = WG.open_rw(ctx, s)
    try:
        for sp, want in ((49, [b"d"]), (50, [b"c", b"d"]), (U64, [b"c", b"d"])):  # start_ts == safe_point refuses
            m = W.clone(s)
            nxt, got = MG.step(ms, m, ("gc", b"b", b"", sp))
            assert nxt is None and got == ("locked", want)
            with pytest.raises(M.ErrGCLocked) as e:
                ms.gc(b"b", b"", sp)
            assert e.value.Key == want[0] and ms.last_maint["first_error"] == sorted(s.locks).index(want[0])
        m = W.clone(s)
        nxt, got = MG.step(ms, m, ("gc", b"b", b"", 39))  # safe_point + 1 does not refuse; a's lock at 5 is outside the range
        assert got == ("ok", True) and m.versions[b"a"] == s.versions[b"a"] and len(m.versions[b"d"]) == 1
        nxt.close()
        m = W.clone(s)
        nxt, got = MG.step(ms, m, ("gc", b"", b"", 4))
        assert got == ("ok", True)
        nxt.close()
        m = W.clone(s)
        assert MG.step(ms, m, ("gc", b"", b"", 5))[1] == ("locked", [b"a"])
    finally:
        ms.close()


# ---------------------------------------------------------------- range edges, for all calls
def range_store():
    s = R.Store()
    for i, k in enumerate((b"4", b"4\x00", b"5", b"k" * 300, b"q", b"x")):
        s.versions[k] = [V(PUT, 7, 8, b"new%d" % i), V(R.ROLLBACK, 6, 6, b""), V(PUT, 3, 4, b"old")]
    for k, st in ((b"1", 9), (b"4\x00", 9), (b"5", 12), (b"k" * 300, 9), (b"zz", 9)):  # lock-only keys first and last
        s.locks[k] = R.Lock(st, b"1", b"lv-" + k[:2], PUT, 1)
    return s


RANGES = [(b"", b""), (b"", b"5"), (b"4", b""), (b"5", b"5"), (b"4", b"4\x00"), (b"4\x00", b"5"), (b"41", b"42"), (b"6", b"j"), (b"9", b"2"), (b"1", b"zz"),
          (b"1", b"zz\x00"), (b"0", b"1"), (b"0", b"1\x00"), (b"k" * 299, b"k" * 301), (b"x", b""), (b"zz", b"")]


@pytest.mark.parametrize("rng_i", range(len(RANGES)))
def test_range_edges_for_all_calls(ctx, rng_i):
    a, b = RANGES[rng_i]
    s = range_store()
    ms = WG.open_rw(ctx, s)
    try:
        for call in (("scan_lock", a, b, 9), ("scan_lock", a, b, U64), ("resolve", a, b, {9: 11}), ("resolve", a, b, {9: 0, 12: 13}), ("gc", a, b, 8), ("gc", a, b, 9),
                     ("delete_range", a, b)):
            m = W.clone(s)
            nxt, want = MG.step(ms, m, call)
            if call[0] == "delete_range" and b == b"":
                assert nxt is None and want is False  # an empty end deletes NOTHING (EncodeBytes("") sorts under every key)
            if call == ("resolve", b"", b"", {9: 11}):
                assert nxt is not None and len(m.locks) == 1
            if nxt is not None:
                nxt.close()
    finally:
        ms.close()


def test_delete_range_empty_end_departs_from_the_other_three(ctx):
    s = range_store()
    ms = WG.open_rw(ctx, s)
    try:
        assert ms.delete_range(b"", b"") is ms and ms.delete_range(b"4", b"") is ms and ms.last_maint["versions_removed"] == 0
        assert len(ms.scan_lock(b"4", b"", U64)) == 4  # unbounded for ScanLock
        nxt = ms.resolve_lock(b"4", b"", 9, 0)  # ... for ResolveLock
        assert nxt is not ms and nxt.n_locks == 2
        nxt.close()
        nxt = ms.gc(b"4", b"", 8)  # ... and for GC
        assert nxt is not ms and nxt.n == 6
        nxt.close()
        nxt = ms.delete_range(b"", b"\xff")  # an empty start is the first key
        assert nxt.n == 0 and nxt.n_locks == 0
        nxt.close()
    finally:
        ms.close()


# ---------------------------------------------------------------- resolve
def test_resolve_ops_placement_and_replacement(ctx):
    s = R.Store()
    s.versions[b"mid"] = [V(PUT, 29, 30, b"c"), V(PUT, 19, 20, b"b"), V(PUT, 9, 10, b"a")]
    s.versions[b"rep"] = [V(PUT, 29, 30, b"c"), V(PUT, 19, 25, b"replaced"), V(PUT, 9, 10, b"a")]
    s.versions[b"rb"] = [V(PUT, 29, 30, b"c"), V(PUT, 7, 21, b"at-start-ts"), V(PUT, 9, 10, b"a")]
    for k, op, val in ((b"del", DEL, b""), (b"lock", LOCK, b""), (b"mid", PUT, b"m21"), (b"rb", PUT, b"r21"), (b"rep", PUT, b"p21")):
        s.locks[k] = R.Lock(21, b"del", val, op, 0)
    t = run(ctx, s, [("resolve", b"", b"rb", {21: 25})])
    assert t.versions[b"del"] == [V(DEL, 21, 25, b"")] and b"lock" not in t.versions and b"lock" not in t.locks  # Op_Del: a DELETE; Op_Lock: no version
    assert [v.value for v in t.versions[b"mid"]] == [b"c", b"m21", b"b", b"a"] and sorted(t.locks) == [b"rb", b"rep"]  # the middle of a chain
    t = run(ctx, s, [("resolve", b"rep", b"", {21: 25})])
    assert t.versions[b"rep"] == [V(PUT, 29, 30, b"c"), V(PUT, 21, 25, b"p21"), V(PUT, 9, 10, b"a")]  # an equal commitTS is replaced
    t = run(ctx, s, [("resolve", b"rb", b"rc", {21: 0})])
    assert t.versions[b"rb"] == [V(PUT, 29, 30, b"c"), V(R.ROLLBACK, 21, 21, b""), V(PUT, 9, 10, b"a")]  # ... and an equal (key, startTS) by a rollback
    ms = WG.open_rw(ctx, s)
    try:
        nxt = ms.resolve_lock(b"", b"", 21, 25)
        assert ms.last_maint["versions_added"] == 4 and ms.last_maint["versions_replaced"] == 1 and ms.last_maint["locks_removed"] == 5
        nxt.close()
    finally:
        ms.close()


def test_resolve_lock_values_at_the_wave_copy_threshold(ctx):
    s = R.Store()
    for i, n in enumerate((0, 1, 63, 64, 300)):
        s.locks[b"v%d" % i] = R.Lock(5, b"v0", bytes(range(256)) * 2 if n == 300 else b"y" * n, DEL if n == 0 else PUT, 0)
        s.locks[b"v%d" % i] = s.locks[b"v%d" % i]._replace(value=s.locks[b"v%d" % i].value[:n])
    t = run(ctx, s, [("resolve", b"", b"", {5: 6})])
    assert [len(t.versions[b"v%d" % i][0].value) for i in range(5)] == [0, 1, 63, 64, 300] and not t.locks


def test_resolve_transaction_lists(ctx):
    s = R.Store()
    for i in range(200):  # two transactions' locks interleaved in key order, a third beside them
        s.locks[b"k%03d" % i] = R.Lock(100 + i % 3, b"k000", b"v%d" % i, PUT, 0)
    s.versions[b"k005"] = [V(PUT, 1, 2, b"x")]
    assert run(ctx, s, [("resolve", b"", b"", {})]).locks == s.locks  # 0 transactions
    t = run(ctx, s, [("resolve", b"", b"", {100: 200})])  # 1
    assert len(t.locks) == 133 and t.versions[b"k003"] == [V(PUT, 100, 200, b"v3")]
    infos = {1000 + i: 5 for i in range(63)}  # 65 in the list, 63 of them without locks
    infos.update({101: 0, 100: 300})
    t = run(ctx, s, [("resolve", b"k010", b"k150", infos)])
    assert len(t.locks) == 200 - 93 and t.versions[b"k010"] == [V(R.ROLLBACK, 101, 101, b"")] and t.versions[b"k012"] == [V(PUT, 100, 300, b"v12")]
    assert run(ctx, s, [("resolve", b"", b"", {77: 78, 99: 0})]).locks == s.locks  # listed transactions without locks


def test_resolve_refusals(ctx):
    s = range_store()
    ms = WG.open_rw(ctx, s)
    try:
        for pairs, text in (([(9, 10), (9, 0)], "given twice"), ([(9, U64)], "2^64 - 1"), ([(U64, 0)], "2^64 - 1"), ([(3, 4), (9, 10), (5, 6), (9, 10)], "given twice")):
            with pytest.raises(_lib.TsqError) as e:
                ms.batch_resolve_lock(b"", b"", pairs)
            assert e.value.status == abi.ERR_INVALID and text in e.value.message
        WG.compare_store(ms, s)
        nxt = ms.batch_resolve_lock(b"", b"", [(12, 13), (9, 10)])  # unsorted is the host side's to sort
        assert nxt.n_locks == 0
        nxt.close()
        nxt = ms.batch_resolve_lock(b"", b"", [(U64, 5), (9, U64 - 1)])
        assert nxt.n_locks == 1
        nxt.close()
    finally:
        ms.close()


# ---------------------------------------------------------------- handles
def test_a_plain_store_refuses_the_mutating_calls_and_answers_scan_lock(ctx):
    s = range_store()
    ps = G.open_store(ctx, W.clone(s))
    try:
        assert [l.fields() for l in ps.scan_lock(b"", b"", 9)] == MM.scan_lock(s, b"", b"", 9) and len(ps.scan_lock(b"5", b"", U64)) == 3
        for f in (lambda: ps.resolve_lock(b"", b"", 9, 10), lambda: ps.gc(b"", b"", 100), lambda: ps.delete_range(b"", b"z")):
            with pytest.raises(_lib.TsqError) as e:
                f()
            assert e.value.status == abi.ERR_INVALID and "tsq_mvcc_create_rw" in e.value.message
    finally:
        ps.close()


def test_changed_nothing_returns_null_old_handle_reads_unchanged_next_outlives_it(ctx):
    rng = np.random.default_rng(19)
    s = W.writable_random_store(rng, 100)
    old = W.clone(s)
    ms = WG.open_rw(ctx, s)
    res, nxt = abi.MvccMaintResult(), C.c_void_p(1)
    st = np.array([123456], dtype=np.uint64)
    assert ms.lib.tsq_mvcc_resolve_lock(ms.h, None, 0, None, 0, st.ctypes.data, st.ctypes.data, 1, C.byref(res), C.byref(nxt)) == abi.OK and nxt.value is None
    nxt = C.c_void_p(1)
    assert ms.lib.tsq_mvcc_delete_range(ms.h, b"\xff\xff", 2, b"\xff\xff\xff", 3, C.byref(res), C.byref(nxt)) == abi.OK and nxt.value is None
    assert (res.versions_removed, res.locks_removed, res.n_errors, res.first_error) == (0, 0, 0, -1)
    a, _ = MG.step(ms, s, ("resolve", b"", b"", {l.start_ts: l.start_ts + 1 for l in s.locks.values() if l.start_ts < U64 - 1}))
    b, _ = MG.step(a, s, ("gc", b"", b"", U64))
    WG.compare_store(ms, old)
    G.check(ms, old, [(b"", b"")], U64 - 1)
    ms.close()
    a.close()
    G.check(b, s, [(b"", b"")], U64 - 1)
    c, _ = MG.step(b, s, ("delete_range", s.keys()[10], s.keys()[20]))
    c.cancel()
    for f in (lambda: c.scan_lock(b"", b"", 5), lambda: c.resolve_lock(b"", b"", 1, 2), lambda: c.gc(b"", b"", 5), lambda: c.delete_range(b"a", b"b")):
        with pytest.raises(_lib.TsqError) as e:
            f()
        assert e.value.status == abi.ERR_CANCELLED
    c.close()
    b.close()


def test_device_resident_scan_lock_output_equals_the_host_resident_one(ctx):
    rng = np.random.default_rng(23)
    s = W.writable_random_store(rng, 500)
    for i in range(150):
        s.locks[b"L%04d" % i + b"x" * (i % 90)] = R.Lock(int(rng.integers(0, 100)), b"P" * (i % 70), b"v", PUT, 0)
    ms = WG.open_rw(ctx, s)
    try:
        for a, b, ts in ((b"", b"", U64), (b"L0050", b"L0120", 50), (b"zzz", b"", U64)):
            host = ms.scan_lock_packed(a, b, ts)
            dev = ms.scan_lock_packed(a, b, ts, device=True)
            try:
                n = host[0]
                assert dev[0] == n == len(MM.scan_lock(s, a, b, ts))
                for h, d, cnt in zip(host[1:], dev[1:], (ms.last_scan_lock["key_bytes"], n + 1, ms.last_scan_lock["primary_bytes"], n + 1, n, n)):
                    assert np.array_equal(h[:cnt], d.read(h.dtype, cnt)), (a, b)
            finally:
                for d in dev[1:]:
                    d.free()
    finally:
        ms.close()


def test_arena_returns_to_its_start_after_calls_with_and_without_errors():
    actx = _lib.Context(0)
    try:
        actx.reserve(256 << 20)
        rng = np.random.default_rng(2)
        s = W.writable_random_store(rng, 300)
        s.locks[b"low"] = R.Lock(0, b"low", b"v", PUT, 0)
        ms = WG.open_rw(actx, s)
        n_scan = len(ms.scan_lock(b"", b"", U64))  # (its output stays with the handle, as a scan's does)
        start = actx.arena_stats()["used"]
        assert start > 0 and n_scan == len(s.locks)
        for i in range(10):
            with pytest.raises(M.ErrGCLocked):
                ms.gc(b"", b"", 5 + i)  # refused: nothing is written
            with pytest.raises(_lib.TsqError):
                ms.batch_resolve_lock(b"", b"", [(7, 8), (7, 9)])
            assert ms.resolve_lock(b"", b"", 987654 + i, 0) is ms and ms.delete_range(b"\xff\xfe", b"\xff\xff") is ms and ms.gc(b"\xff\xfe", b"", U64) is ms
            assert len(ms.scan_lock(b"", b"", U64)) == n_scan
        assert actx.arena_stats()["used"] == start
        for i in range(5):
            a = ms.batch_resolve_lock(b"", b"", {l.start_ts: 0 for l in s.locks.values()})
            b = a.gc(b"", b"", 1 << 62)
            c = b.delete_range(b"A", b"B")
            assert a is not ms and b is not a and c is not b
            for h in (a, b, c):
                h.close()
        assert actx.arena_stats()["used"] == start and actx.arena_stats()["peak"] > start
        ms.close()
        assert actx.arena_stats()["used"] == 0
    finally:
        actx.close()
