"""GPU parity of the MVCC writes (tsq_mvcc_create_rw / prewrite / commit / rollback / lock_at / sizes / export) with the sequential
model of tests/mvcc_write_ref.py: after every write the verdict of every key with its fields, the full export against the model's
arrays plus lock values, then reads against mvcc_ref.read_ranges."""
import ctypes as C
import json
import os

import numpy as np
import pytest

from tests import mvcc_gpu_helpers as G
from tests import mvcc_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import mvcc_write_ref as W
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import mvcc as M
from tinysql_amd.dupcheck import DevArray

pytestmark = pytest.mark.gpu

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = lambda s: s.encode("latin-1")
U64 = R.U64_MAX
PUT, DEL, LOCK = R.OP_PUT, R.OP_DEL, R.OP_LOCK


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "mvcc_write_cases.json")))["cases"]


def step_call(st):
    if st["op"] == "prewrite":
        return ("prewrite", [(R.OP_NAMES[m[0]], L1(m[1]), L1(m[2])) for m in st["mutations"]], L1(st["primary"]), st["start_ts"], st["ttl"])
    if st["op"] == "commit":
        return ("commit", [L1(k) for k in st["keys"]], st["start_ts"], st["commit_ts"])
    return ("rollback", [L1(k) for k in st["keys"]], st["start_ts"])


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_the_references_write_steps(ctx, case):
    s = R.Store()
    ms = WG.open_rw(ctx, s)
    try:
        for st in case["steps"]:
            if st["op"] == "noop":
                continue
            if st["op"] == "get":
                got = G.check(ms, s, [(L1(st["key"]), None)], st["ts"])
                assert (got[0] == "locked") if st["err"] else (got == ("ok", [] if st["expect"] is None else [(L1(st["key"]), L1(st["expect"]))], [0 if st["expect"] is None else 1])), st["line"]
                continue
            nxt, verdicts = WG.step(ms, s, step_call(st))
            assert [v[0] for v in verdicts] == [W.NAMES[x] for x in st["verdicts"]], st["line"]
            assert (nxt is not None) == (st["asserts"] == "ok"), st["line"]
            if nxt is not None:
                ms.close()
                ms = nxt
    finally:
        ms.close()


# ---------------------------------------------------------------- random histories
@pytest.mark.parametrize("style", ["prefix", "record"])
@pytest.mark.parametrize("n_keys", [0, 1, 63, 64, 65, 2047, 2048, 2049])
def test_random_histories(ctx, n_keys, style):
    rng = np.random.default_rng(1000 + n_keys + (7 if style == "record" else 0))
    s = W.writable_random_store(rng, n_keys, style)
    fresh = [b"\x01first", b"Bmid", b"zz-last", b"\x01first\x00", b"Bmie"]
    assert not set(fresh) & set(s.keys())
    txns = [30, 35, 1001, (1 << 63) + 5]
    n_random = int(rng.integers(11, 32))  # 20 .. 40 calls with the nine scripted ones
    big = n_keys > 1000
    calls = W.scripted_calls(*fresh[:3]) + [lambda st: W.random_call(st, rng, txns, fresh)] * n_random
    ms, kinds = WG.run_calls(ctx, s, calls, reads=not big)
    try:
        assert kinds == W.ALL_KINDS, W.ALL_KINDS - kinds
        G.check(ms, s, [(b"", b"")], U64 - 1)
        for r in R.random_ranges(s, rng, 4):
            G.check(ms, s, [r], 1001)
    finally:
        ms.close()


# ---------------------------------------------------------------- request shapes at a fixed store
def shape_store():
    rng = np.random.default_rng(77)
    s = R.Store()
    for key in R.random_keys(rng, 300, "record"):
        s.versions[key] = [R.Value(R.PUT, 8, 9, b"nine-" + key[-2:]), R.Value(R.PUT, 3, 4, b"four")][:int(rng.integers(1, 3))]
    return s


def shape_keys(s, shape, n):
    ks = s.keys()
    if shape == "before":
        return [b"a%06d" % i for i in range(n)]
    if shape == "behind":
        return [b"u%06d" % i for i in range(n)]
    if shape == "existing":
        return [ks[i % len(ks)] + (b"" if i < len(ks) else b"\x00%05d" % i) for i in range(n)]
    if shape == "every_second_new":
        return [ks[(i // 2) % len(ks)] + (b"" if i % 2 == 0 and i // 2 < len(ks) else b"\x00%05d" % i) for i in range(n)]
    assert shape == "between_two"  # all between ks[7] and ks[8]
    return [ks[7] + b"\x00%06d" % i for i in range(n)]


@pytest.mark.parametrize("shape", ["before", "behind", "existing", "every_second_new", "between_two"])
@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 2049])
def test_request_shapes(ctx, n, shape):
    s = shape_store()
    keys = sorted(set(shape_keys(s, shape, n)))
    assert len(keys) == n
    muts = [(PUT if i % 3 else DEL, k, b"v%d" % i if i % 3 else b"") for i, k in enumerate(keys)]
    calls = [("prewrite", muts, keys[0] if keys else b"p", 20, 3), ("commit", keys[: n // 2 + 1] if n else [], 20, 25), ("rollback", keys[n // 2 + 1:], 20)]
    ms, kinds = WG.run_calls(ctx, s, calls, reads=n <= 65)
    try:
        assert not kinds and ms.n_locks == 0
        G.check(ms, s, [(b"", b"")], 25)
        G.check(ms, s, [(b"", b"")], 24)
    finally:
        ms.close()


# ---------------------------------------------------------------- edges
def history(ctx, s, calls, want_kinds=()):
    ms, kinds = WG.run_calls(ctx, s, calls)
    assert kinds == set(want_kinds), kinds
    return ms


def test_start_ts_zero_on_an_absent_key_conflicts_with_fields_zero(ctx):
    s = R.Store()
    s.put(b"k", b"v", 1, 2)
    ms = WG.open_rw(ctx, s)
    try:
        with pytest.raises(M.ErrConflict) as e:
            ms.prewrite([(PUT, b"absent", b"x"), (PUT, b"k", b"y")], b"absent", 0)
        assert (e.value.StartTS, e.value.ConflictTS, e.value.ConflictCommitTS, e.value.Key) == (0, 0, 0, b"absent")
        assert [type(x) for x in e.value.errors] == [M.ErrConflict, M.ErrConflict] and e.value.errors[1].ConflictCommitTS == 2
        nxt = ms.prewrite([(PUT, b"absent", b"x")], b"absent", 1)
        nxt.close()
    finally:
        ms.close()


def test_unsigned_timestamp_order(ctx):
    s = R.Store()
    s.put(b"k", b"small", 5, 6)
    big = (1 << 63) + 9
    ms = history(ctx, s, [("prewrite", [(PUT, b"k", b"big")], b"k", big, 0), ("commit", [b"k"], big, big + 1),  # lands in front of commitTS 6
                          ("prewrite", [(PUT, b"k", b"late")], b"k", (1 << 63) - 1, 0),  # 2^63 + 10 >= 2^63 - 1: conflict
                          ("prewrite", [(PUT, b"k", b"mid")], b"k", U64 - 1, 0), ("rollback", [b"k"], U64 - 1)], ["conflict"])
    try:
        assert [v.commit_ts for v in s.versions[b"k"]] == [U64 - 1, big + 1, 6]
        assert ms.get(b"k", big) == b"small" and ms.get(b"k", big + 1) == b"big"
    finally:
        ms.close()


def test_commit_replaces_an_equal_commit_ts_and_lands_in_the_middle_of_a_chain(ctx):
    s = R.Store()
    s.versions[b"k"] = [R.Value(R.PUT, 40, 50, b"fifty"), R.Value(R.ROLLBACK, 30, 30, b""), R.Value(R.PUT, 10, 20, b"twenty")]
    s.versions[b"m"] = [R.Value(R.PUT, 10, 20, b"m20")]
    s.locks[b"k"] = R.Lock(25, b"k", b"new-30", PUT, 0)  # committed at 30: the rollback version of 30 is replaced
    s.locks[b"m"] = R.Lock(12, b"k", b"m15", PUT, 0)  # committed at 15: behind commitTS 20
    ms = WG.open_rw(ctx, s)
    try:
        nxt, _ = WG.step(ms, s, ("commit", [b"k"], 25, 30))
        assert nxt.last_write["versions_added"] == 1 and nxt.last_write["versions_replaced"] == 1 and nxt.last_write["locks_removed"] == 1
        assert [(v.type, v.commit_ts) for v in s.versions[b"k"]] == [(R.PUT, 50), (R.PUT, 30), (R.PUT, 20)] and nxt.get(b"k", 35) == b"new-30"
        nx2, _ = WG.step(nxt, s, ("commit", [b"m"], 12, 15))
        assert nx2.last_write["versions_replaced"] == 0 and [v.commit_ts for v in s.versions[b"m"]] == [20, 15]
        s2 = W.clone(s)
        s2.locks[b"k"] = R.Lock(41, b"k", b"between", PUT, 0)  # 50 > 45 > 30: the middle of the chain
        mid = WG.open_rw(ctx, s2)
        nx3, _ = WG.step(mid, s2, ("commit", [b"k"], 41, 45))
        assert [v.commit_ts for v in s2.versions[b"k"]] == [50, 45, 30, 20]
        for h in (nx3, mid, nx2, nxt):
            h.close()
    finally:
        ms.close()


def test_rollback_beside_a_foreign_lock_op_lock_commit_del_commit_and_own_lock_replaced(ctx):
    s = R.Store()
    s.put(b"d", b"dv", 1, 2)
    calls = [("prewrite", [(PUT, b"f", b"foreign")], b"f", 10, 0),
             ("rollback", [b"f"], 11),  # no version of 11, a foreign lock: the rollback version is added, the lock stays
             ("prewrite", [(LOCK, b"l", b"")], b"l", 12, 0), ("commit", [b"l"], 12, 13),  # lock gone, no version
             ("prewrite", [(DEL, b"d", b"")], b"d", 14, 0), ("commit", [b"d"], 14, 15),
             ("prewrite", [(PUT, b"o", b"one")], b"o", 16, 1), ("prewrite", [(PUT, b"o", b"another value")], b"o2", 16, 2)]
    ms = history(ctx, s, calls)
    try:
        assert s.locks[b"f"].start_ts == 10 and s.versions[b"f"] == [R.Value(R.ROLLBACK, 11, 11, b"")]
        assert b"l" not in s.locks and b"l" not in s.versions
        assert ms.get(b"d", 15) is None and ms.get(b"d", 14) == b"dv"
        assert s.locks[b"o"] == R.Lock(16, b"o2", b"another value", PUT, 2) and ms.last_write["locks_added"] == 1 and ms.last_write["locks_removed"] == 1
    finally:
        ms.close()


@pytest.mark.parametrize("n", [63, 64, 65, 300])
def test_long_chains_wanted_start_ts_last_and_absent(ctx, n):
    s = R.Store()
    s.versions[b"hot"] = [R.Value(R.PUT, 10 * c, 10 * c + 1, b"h") for c in range(n, 1, -1)] + [R.Value(R.PUT, 7, 8, b"first")]
    s.versions[b"rolled"] = [R.Value(R.PUT, 10 * c, 10 * c + 1, b"h") for c in range(n, 1, -1)] + [R.Value(R.ROLLBACK, 7, 7, b"")]
    s.versions[b"other"] = [R.Value(R.PUT, 10 * c, 10 * c + 1, b"h") for c in range(n, 0, -1)]
    calls = [("commit", [b"hot", b"other", b"rolled"], 7, 9), ("commit", [b"hot"], 7, 9), ("rollback", [b"hot"], 7), ("rollback", [b"other", b"rolled"], 7),
             ("rollback", [b"other"], 10 * n + 5), ("rollback", [b"other"], 15)]
    ms = history(ctx, s, calls, ["txn_not_found", "already_committed", "noop_commit", "noop_rollback"])
    ms.close()
    # the lane form gives the same (the threshold knob off)
    ctx.set_knob(abi.KNOB_MVCC_WAVE_CHAIN, 0)
    s2 = R.Store()
    s2.versions[b"hot"] = [R.Value(R.PUT, 10 * c, 10 * c + 1, b"h") for c in range(n, 1, -1)] + [R.Value(R.PUT, 7, 8, b"first")]
    ms = history(ctx, s2, [("rollback", [b"hot"], 7), ("commit", [b"hot"], 7, 9), ("commit", [b"hot"], 6, 9)], ["txn_not_found", "already_committed", "noop_commit"])
    ms.close()


def test_value_and_key_lengths(ctx):
    s = R.Store()
    s.put(b"k" * 300, b"old" * 30, 1, 2)
    sizes = [1, 63, 64, 65, 5000]
    keys = [b"v%04d" % n for n in sizes] + [b"k" * 300, b"q"]
    muts = [(PUT, b"v%04d" % n, bytes(np.arange(n, dtype=np.uint8) % 251)) for n in sizes] + [(DEL, b"k" * 300, b""), (PUT, b"q", b"1")]
    ms = history(ctx, s, [("prewrite", muts, b"p" * 200, 10, 0), ("commit", keys, 10, 11)])
    try:
        assert ms.get(b"v5000", 11) == bytes(np.arange(5000, dtype=np.uint8) % 251) and ms.get(b"k" * 300, 11) is None and ms.get(b"k" * 300, 10) == b"old" * 30
    finally:
        ms.close()


# ---------------------------------------------------------------- refusals
def packed_req(keys, ops=None, values=None, primary=b"p", start_ts=10, commit_ts=11, ttl=0, keep=None):
    kb, ko = M._pack_cells(list(keys))
    req = abi.MvccWriteReq()
    keep += [kb, ko]
    req.keys, req.key_offsets, req.key_bytes, req.n_keys = (kb.ctypes.data if kb.size else None), ko.ctypes.data, kb.size, len(keys)
    if ops is not None:
        o = np.array(ops, dtype=np.uint8)
        vb, vo = M._pack_cells(list(values))
        pr = np.frombuffer(primary, dtype=np.uint8).copy()
        keep += [o, vb, vo, pr]
        req.ops, req.values, req.value_offsets, req.value_bytes = o.ctypes.data, (vb.ctypes.data if vb.size else None), vo.ctypes.data, vb.size
        req.primary, req.primary_len = pr.ctypes.data, pr.size
    req.start_ts, req.commit_ts, req.ttl = start_ts, commit_ts, ttl
    return req


def refused(ms, kind, req, n, status, text):
    with pytest.raises(_lib.TsqError) as e:
        ms.write_packed(kind, req, n)
    assert e.value.status == status and text in e.value.message, e.value.message


def test_refusals_leave_no_next_store_and_the_store_reads_as_before(ctx):
    s = R.Store()
    s.put(b"b", b"bv", 1, 2)
    s.prewrite([(PUT, b"c", b"cv")], b"c", 5)
    ms = WG.open_rw(ctx, s)
    keep = []
    INV = abi.ERR_INVALID
    try:
        refused(ms, "prewrite", packed_req([b"b", b"a"], [0, 0], [b"x", b"y"], keep=keep), 2, INV, "mvcc write: keys not strictly ascending")
        refused(ms, "commit", packed_req([b"a", b"a"], keep=keep), 2, INV, "mvcc write: keys not strictly ascending")
        refused(ms, "rollback", packed_req([b"", b"a"], keep=keep), 2, INV, "mvcc write: empty key")
        refused(ms, "prewrite", packed_req([b"a"], [3], [b"x"], keep=keep), 1, INV, "mvcc write: a prewrite op other than Put, Del or Lock")
        refused(ms, "prewrite", packed_req([b"a"], [0], [b""], keep=keep), 1, INV, "mvcc write: a put with an empty value")
        refused(ms, "commit", packed_req([b"a"], commit_ts=U64, keep=keep), 1, INV, "mvcc write: commitTS 2^64 - 1 is the lock's version")
        refused(ms, "rollback", packed_req([b"a"], start_ts=U64, keep=keep), 1, INV, "mvcc write: commitTS 2^64 - 1 is the lock's version")
        for bad in ([0, 3, 2], [0, 1, 9], [-1, 1, 2]):  # offsets that decrease, leave the buffer, start below it
            req = packed_req([b"a", b"b"], keep=keep)
            ko = np.array(bad, dtype=np.int64)
            keep.append(ko)
            req.key_offsets = ko.ctypes.data
            refused(ms, "commit", req, 2, INV, "mvcc write: offsets decrease or leave their buffer")
        req = packed_req([b"a", b"d"], [0, 0], [b"x", b"y"], keep=keep)
        vo = np.array([0, 3, 2], dtype=np.int64)
        keep.append(vo)
        req.value_offsets = vo.ctypes.data
        refused(ms, "prewrite", req, 2, INV, "mvcc write: offsets decrease or leave their buffer")
        # 2^31 entries: decided before any array is read — the pointers are not memory
        req = abi.MvccWriteReq()
        req.keys, req.key_offsets, req.key_bytes, req.n_keys = 8, 8, 1 << 40, (1 << 31) - ms.n - ms.n_locks  # n + n_locks + n_keys = 2^31
        refused(ms, "commit", req, 0, abi.ERR_UNSUPPORTED, "mvcc write: 2^31 entries or more")
        WG.compare_store(ms, s)
        G.check(ms, s, [(b"", b"")], 3)
        G.check(ms, s, [(b"", b"")], 9)
    finally:
        ms.close()


def test_plain_store_refuses_writes_and_rw_create_refuses_an_empty_put_lock(ctx):
    s = R.Store()
    s.put(b"b", b"bv", 1, 2)
    plain = G.open_store(ctx, W.clone(s))
    keep = []
    try:
        refused(plain, "commit", packed_req([b"b"], keep=keep), 1, abi.ERR_INVALID, "mvcc write: the store was created without start_ts and lock values")
        with pytest.raises(_lib.TsqError):
            plain.export()
    finally:
        plain.close()
    s.locks[b"e"] = R.Lock(5, b"e", b"", PUT, 0)
    with pytest.raises(_lib.TsqError) as e:
        WG.open_rw(ctx, s)
    assert e.value.status == abi.ERR_INVALID and "mvcc store: a put lock with an empty value" in e.value.message
    s.locks[b"e"] = R.Lock(5, b"e", b"", DEL, 0)
    f = W.flat_rw(s)
    f["lock_value_offsets"] = np.array([0, 4], dtype=np.int64)
    with pytest.raises(_lib.TsqError) as e:
        M.MvccStore.create_rw(ctx, f)
    assert "mvcc store: offsets decrease or leave their buffer" in e.value.message
    f = W.flat_rw(s)
    del f["start_ts"]
    with pytest.raises(_lib.TsqError) as e:
        M.MvccStore.create_rw(ctx, f)
    assert "a writable store needs start_ts" in e.value.message
    WG.open_rw(ctx, s).close()


def test_reads_on_a_writable_store_equal_reads_on_a_plain_one(ctx):
    rng = np.random.default_rng(12)
    s = W.writable_random_store(rng, 200)
    a, b = WG.open_rw(ctx, s), G.open_store(ctx, W.clone(s))
    try:
        for ts in R.read_timestamps(s, rng, 4):
            for r in R.random_ranges(s, rng, 4):
                assert G.gpu_answer(a, [r], ts) == G.gpu_answer(b, [r], ts)
    finally:
        a.close()
        b.close()


# ---------------------------------------------------------------- device-resident requests
def test_device_resident_requests_give_the_same_next_store(ctx):
    rng = np.random.default_rng(5)
    s = W.writable_random_store(rng, 100)
    keys = sorted(set(s.keys()[::7]) - set(s.locks)) + [b"zz%03d" % i for i in range(70)]
    ok = [k for k in keys if W.prewrite_verdict(s, k, U64 - 5)[0] == W.OK]
    ops, vals = [PUT if i % 2 else DEL for i in range(len(ok))], [b"dev%d" % i if i % 2 else b"" for i in range(len(ok))]
    keep, devs = [], []
    ms = WG.open_rw(ctx, s)
    try:
        host = packed_req(ok, ops, vals, primary=ok[0], start_ts=U64 - 5, ttl=4, keep=keep)
        dev = packed_req(ok, ops, vals, primary=ok[0], start_ts=U64 - 5, ttl=4, keep=keep)
        for name, arr in (("keys", keep[-6]), ("key_offsets", keep[-5]), ("ops", keep[-4]), ("values", keep[-3]), ("value_offsets", keep[-2])):
            d = DevArray(ctx, arr)
            devs.append(d)
            setattr(dev, name, d.p)
        dev.flags = abi.COL_DEVICE
        a, va, ia, _ = ms.write_packed("prewrite", host, len(ok))
        b, vb, ib, _ = ms.write_packed("prewrite", dev, len(ok))
        assert a is not None and b is not None and np.array_equal(va, vb) and np.array_equal(ia, ib)
        assert W.same_flat(a.export(), b.export()) is None
        W.prewrite(s, list(zip(ops, ok, vals)), ok[0], U64 - 5, 4)
        WG.compare_store(b, s)
        dev.commit_ts = host.commit_ts = U64 - 4
        a2, _, _, _ = a.write_packed("commit", host, len(ok))
        b2, _, _, _ = b.write_packed("commit", dev, len(ok))
        W.commit(s, ok, U64 - 5, U64 - 4)
        WG.compare_store(a2, s)
        WG.compare_store(b2, s)
        for h in (a, b, a2, b2):
            h.close()
    finally:
        ms.close()
        for d in devs:
            d.free()


# ---------------------------------------------------------------- lifetime
def test_old_handle_reads_unchanged_and_the_next_outlives_it(ctx):
    rng = np.random.default_rng(9)
    s = W.writable_random_store(rng, 100)
    old = W.clone(s)
    ms = WG.open_rw(ctx, s)
    nxt, _ = WG.step(ms, s, ("prewrite", [(PUT, b"new", b"n1")], b"new", 9000, 0))
    nx2, _ = WG.step(nxt, s, ("commit", [b"new"], 9000, 9001))
    WG.compare_store(ms, old)
    G.check(ms, old, [(b"", b"")], 9001)
    ms.close()
    nxt.close()
    G.check(nx2, s, [(b"", b"")], 9001)
    assert nx2.get(b"new", 9001) == b"n1" and nx2.get(b"new", 9000) is None
    empty, _ = WG.step(nx2, s, ("commit", [], 1, 2))  # an empty request: a next store equal to the current one
    assert empty.last_write["versions_added"] == 0
    empty.cancel()
    for f in (lambda: empty.get(b"new", 9001), lambda: empty.commit([b"new"], 1, 2), empty.export, lambda: empty.lock_at(0)):
        with pytest.raises(_lib.TsqError) as e:
            f()
        assert e.value.status == abi.ERR_CANCELLED
    empty.close()
    assert nx2.get(b"new", 9001) == b"n1"
    nx2.close()


def test_arena_returns_to_its_start_after_writes_with_and_without_errors():
    actx = _lib.Context(0)
    try:
        actx.reserve(256 << 20)
        rng = np.random.default_rng(2)
        s = W.writable_random_store(rng, 300)
        ms = WG.open_rw(actx, s)
        start = actx.arena_stats()["used"]
        assert start > 0
        keep = []
        for i in range(10):
            nxt, _, _, res = ms.write_packed("commit", packed_req([b"nobody%d" % i], start_ts=77, commit_ts=78, keep=keep), 1)
            assert nxt is None and res.n_errors == 1 and res.first_error == 0
            with pytest.raises(_lib.TsqError):
                ms.write_packed("commit", packed_req([b"b", b"a"], keep=keep), 2)
        assert actx.arena_stats()["used"] == start
        for i in range(10):
            nxt = ms.prewrite([(PUT, b"loop%d" % i, b"v")], b"loop", 5000 + i)
            nx2 = nxt.commit([b"loop%d" % i], 5000 + i, 6000 + i)
            nxt.close()
            nx2.close()
        assert actx.arena_stats()["used"] == start and actx.arena_stats()["peak"] > start
        ms.close()
        assert actx.arena_stats()["used"] == 0
    finally:
        actx.close()
