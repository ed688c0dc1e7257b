"""CPU: the model of the MVCC range calls (tests/mvcc_maint_ref.py) against the steps of the reference's own tests
(tests/golden/mvcc_maint_cases.json), the host build of tsq_mvcc_maint_dp.h (sanitized, a stand-alone program) against the model —
the bounds of a range, ScanLock's hits, the plan of every resolved lock applied to the store's arrays, GC's refusal and drops in the
lane and the wave form of the keeper's walk — and the new part of the C-ABI."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mvcc_maint_ref as MM
from tests import mvcc_ref as R
from tests import mvcc_write_ref as W
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = lambda s: s.encode("latin-1")
HEX = lambda b: b.hex() if b else "-"
U64 = R.U64_MAX


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "mvcc_maint_cases.json")))["cases"]


def step_call(st):
    """a golden step as a call tuple of mvcc_maint_ref.apply_call"""
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
    assert st["op"] == "delete_range"
    return ("delete_range", L1(st["start"]), L1(st["end"]))


def check_read_step(s, st):
    """get / scan steps against the model; True when the step was one"""
    if st["op"] == "get":
        assert s.get(L1(st["key"]), st["ts"]) == (None if st["expect"] is None else L1(st["expect"])), st["line"]
        return True
    if st["op"] == "scan":
        got = s.scan(L1(st["start"]), L1(st["end"]), st["limit"], st["ts"])
        assert [(k, v) for k, v, e in got if e is None] == [(L1(k), L1(v)) for k, v in st["expect"]] and all(e is None for _, _, e in got), st["line"]
        return True
    return False


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_model_reproduces_the_references_steps(case):
    s = R.Store()
    calls = 0
    for st in case["steps"]:
        if check_read_step(s, st):
            continue
        call = step_call(st)
        got = MM.apply_call(s, call)
        if call[0] in ("prewrite", "commit"):
            assert got[1] and [v[0] for v in got[0]] == [W.NAMES[x] for x in st["verdicts"]], st["line"]
        elif call[0] == "scan_lock":
            assert got == [(L1(l["primary"]), l["start_ts"], L1(l["key"])) for l in st["expect"]], st["line"]
        elif call[0] == "gc":
            assert got[0] == "ok", st["line"]
        calls += 1
    assert calls >= 4


def test_the_golden_file_holds_the_five_tests():
    n = {c["name"]: sum(1 for st in c["steps"] if st["op"] in ("scan_lock", "resolve", "gc", "delete_range")) for c in golden()}
    assert n == {"TestScanLock": 2, "TestResolveLock": 3, "TestBatchResolveLock": 4, "TestGC": 1, "TestDeleteRange": 5}


def test_model_semantics():
    s = R.Store()
    s.put(b"a", b"a1", 1, 2)
    s.put(b"a", b"a2", 5, 6)
    s.delete(b"b", 3, 4)
    s.prewrite([(R.OP_PUT, b"a", b"a9"), (R.OP_LOCK, b"c", b""), (R.OP_DEL, b"d", b"")], b"a", 9)
    # an empty end: unbounded for the iterator calls, nothing for DeleteRange; an empty start is the first key
    assert len(MM.scan_lock(s, b"", b"", 9)) == 3 and MM.scan_lock(s, b"", b"", 8) == [] and MM.scan_lock(s, b"c", b"c", 9) == []
    assert MM.scan_lock(s, b"b", b"d", U64) == [(b"a", 9, b"c")]
    t = W.clone(s)
    assert not MM.delete_range(t, b"", b"") and not MM.delete_range(t, b"a", b"") and t.versions == s.versions and t.locks == s.locks
    assert MM.delete_range(t, b"", b"b") and sorted(t.versions) == [b"b"] and sorted(t.locks) == [b"c", b"d"]
    assert not MM.delete_range(t, b"c", b"b")
    # GC: the refusal names the locks in key order and writes nothing; unsigned compare
    t = W.clone(s)
    assert MM.gc(t, b"", b"", 9) == ("locked", [b"a", b"c", b"d"]) and MM.gc(t, b"b", b"", 9) == ("locked", [b"c", b"d"]) and t.versions == s.versions
    assert MM.gc(t, b"", b"", 8) == ("ok", True) and t.versions == {b"a": [R.Value(R.PUT, 5, 6, b"a2")]}  # b's delete is the newest: the key goes
    assert MM.gc(t, b"", b"", 8) == ("ok", False)
    # Resolve: Op_Lock commits to no version, Op_Del to a DELETE, a rollback to a ROLLBACK at startTS; a transaction without locks
    t = W.clone(s)
    assert not MM.batch_resolve_lock(t, b"", b"", {8: 20}) and not MM.batch_resolve_lock(t, b"", b"", {})
    assert MM.batch_resolve_lock(t, b"", b"d", {9: 20, 77: 0})
    assert t.versions[b"a"][0] == R.Value(R.PUT, 9, 20, b"a9") and b"c" not in t.versions and sorted(t.locks) == [b"d"]
    assert MM.resolve_lock(t, b"", b"", 9, 0) and t.versions[b"d"] == [R.Value(R.ROLLBACK, 9, 9, b"")] and not t.locks
    u = R.Store()
    u.put(b"k", b"old", 1 << 63, (1 << 63) + 1)
    assert MM.gc(u, b"", b"", (1 << 63)) == ("ok", False) and MM.gc(u, b"", b"", (1 << 63) + 1) == ("ok", False)  # one PUT under the safe point stays


# ------------------------------------------------------------------------------------------------ the host build of tsq_mvcc_maint_dp.h
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mvcc_maint_dp") / "mvcc_maint_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "mvcc_maint_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        return res.stdout.split("\n")
    return run


def store_lines(s):
    out = ["S %d %d" % (sum(len(v) for v in s.versions.values()), len(s.locks))]
    for key in sorted(s.versions):
        for v in s.versions[key]:
            out.append("%s %d %d %d" % (HEX(key), v.commit_ts, v.start_ts, v.type))
    for key in sorted(s.locks):
        out.append("%s %d %d" % (HEX(key), s.locks[key].start_ts, s.locks[key].op))
    return out


def entries(s):
    return [(key, v) for key in sorted(s.versions) for v in s.versions[key]]


def apply_resolve_plan(s, l0, plans):
    """the plan of every lock of the range applied the way tsq_mw_apply does: a new version goes before the entry at its version
    index, a replaced entry goes, a dropped lock goes"""
    lock_keys = sorted(s.locks)
    versions = [(p, 1, key, v) for p, (key, v) in enumerate(entries(s))]
    gone = set()
    for i, (flags, vtype, vsrc, vpos, lpos, vcts) in enumerate(plans):
        key = lock_keys[l0 + i]
        if flags & 2:
            versions = [e for e in versions if not (e[0] == vpos and e[1] == 1)]
        if flags & 1:
            versions.append((vpos, 0, key, R.Value(vtype, s.locks[key].start_ts, vcts, s.locks[lock_keys[vsrc]].value if vsrc >= 0 else b"")))
        assert not flags & 4
        if flags & 8:
            assert lpos == l0 + i
            gone.add(key)
    out = R.Store()
    for _, _, key, v in sorted(versions, key=lambda e: (e[0], e[1])):
        out.versions.setdefault(key, []).append(v)
    out.locks = {k: l for k, l in s.locks.items() if k not in gone}
    return out


def check_call(dp_out, at, s, call, chains):
    """the program's answer to one range call (its lines start at dp_out[at]) against the model; returns (the model after the call,
    the next line)"""
    model = W.clone(s)
    want = MM.apply_call(model, call)
    lock_keys = sorted(s.locks)
    if call[0] == "scan_lock":
        n = int(dp_out[at].split()[1])
        hits = [int(x) for x in dp_out[at + 1].split()]
        assert len(hits) == n and [(s.locks[lock_keys[j]].primary, s.locks[lock_keys[j]].start_ts, lock_keys[j]) for j in hits] == want, call
        return model, at + 2
    if call[0] == "resolve":
        _, l0, q = dp_out[at].split()
        l0, q = int(l0), int(q)
        plans = [tuple(int(x) for x in dp_out[at + 1 + i].split()) for i in range(q)]
        got = apply_resolve_plan(s, l0, plans)
        assert got.versions == model.versions and got.locks == model.locks, call
        assert want == any(p[0] for p in plans)
        for vs in got.versions.values():
            assert all(a.commit_ts > b.commit_ts for a, b in zip(vs, vs[1:]))
        return model, at + 1 + q
    if call[0] == "gc":
        for chain in chains:
            _, nerr, first = dp_out[at].split()
            n = int(dp_out[at + 1].split()[1])
            drops = [int(x) for x in dp_out[at + 2].split()]
            at += 3
            assert len(drops) == n
            if want[0] == "locked":
                assert int(nerr) == len(want[1]) and lock_keys[int(first)] == want[1][0], call
                continue
            assert (int(nerr), int(first)) == (0, -1), call
            got = R.Store()
            for p, (key, v) in enumerate(entries(s)):
                if p not in set(drops):
                    got.versions.setdefault(key, []).append(v)
            assert got.versions == model.versions and want[1] == bool(drops), (call, chain)
        return model, at
    assert call[0] == "delete_range"  # the range test per entry and per lock, on the bounds; an empty end deletes nothing
    u0, u1, e0, e1, l0, l1 = [int(x) for x in dp_out[at].split()[1:]]
    got = R.Store()
    if call[2] == b"":
        e1, l1 = e0, l0
    for p, (key, v) in enumerate(entries(s)):
        if not e0 <= p < e1:
            got.versions.setdefault(key, []).append(v)
    got.locks = {k: s.locks[k] for j, k in enumerate(lock_keys) if not l0 <= j < l1}
    assert got.versions == model.versions and got.locks == model.locks and want == (e1 > e0 or l1 > l0), call
    return model, at + 1


def call_lines(call, chains):
    if call[0] == "scan_lock":
        return ["L %s %s %d" % (HEX(call[1]), HEX(call[2]), call[3])]
    if call[0] == "resolve":
        tx = sorted(call[3].items())
        return ["V %s %s %d" % (HEX(call[1]), HEX(call[2]), len(tx))] + ["%d %d" % t for t in tx]
    if call[0] == "gc":
        return ["G %s %s %d %d" % (HEX(call[1]), HEX(call[2]), call[3], ch) for ch in chains]
    return ["R %s %s" % (HEX(call[1]), HEX(call[2]))]


def run_calls(dp, s, calls, chains=(0, 1)):
    """every call against the store as the calls before it left it (the store is sent again before each)"""
    for call in calls:
        call = call(s) if callable(call) else call
        if call[0] in ("prewrite", "commit", "rollback"):
            W.apply_call(s, call)
            continue
        out = dp(store_lines(s) + call_lines(call, chains))
        assert out[0] == "U %d" % len(s.keys())
        s, _ = check_call(out, 1, s, call, chains)
    return s


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_dp_header_on_the_golden_cases_sanitized(dp, case):
    run_calls(dp, R.Store(), [step_call(st) for st in case["steps"] if st["op"] not in ("get", "scan")])


@pytest.mark.parametrize("n_keys", [0, 1, 65, 2049])
def test_dp_header_against_the_model_on_random_stores_sanitized(dp, n_keys):
    rng = np.random.default_rng(40 + n_keys)
    for style in ("prefix", "record"):
        s = W.writable_random_store(rng, n_keys, style, max_chain=int(rng.choice([1, 5, 9])))
        n_calls = 40 if n_keys < 1000 else 12
        seen = set()
        for _ in range(n_calls):
            call = MM.random_maint_call(s, rng)
            if call[0] == "delete_range" and n_keys > 1 and rng.random() < 0.6:
                continue
            seen.add(call[0])
            s = run_calls(dp, s, [call], (0, 1, 3, 64))
        assert n_calls < 40 or seen == {"scan_lock", "resolve", "gc", "delete_range"}


def chain_store(n, keeper):
    """one key `hot` of n entries under the safe point 10 n + 5: ROLLBACKs with the first non-ROLLBACK — a PUT ("first", "last"), a
    DELETE ("delete_last") or none ("absent") — first or last; "alternating": PUT / ROLLBACK by turns; beside it a short key and a
    version above the safe point"""
    s = R.Store()
    vs = []
    for i in range(n):
        c = 10 * (n - i)
        t = R.ROLLBACK
        if keeper == "alternating":
            t = R.PUT if i % 2 == 0 else R.ROLLBACK
        elif (keeper == "first" and i == 0) or (keeper == "last" and i == n - 1):
            t = R.PUT
        elif keeper == "delete_last" and i == n - 1:
            t = R.DELETE
        vs.append(R.Value(t, c - 1, c, b"p%d" % i if t == R.PUT else b""))
    s.versions[b"hot"] = [R.Value(R.PUT, 10 * n + 8, 10 * n + 9, b"above")] + vs
    s.versions[b"a"] = [R.Value(R.PUT, 1, 2, b"a")]
    s.versions[b"z"] = [R.Value(R.DELETE, 3, 4, b""), R.Value(R.PUT, 1, 2, b"z")]
    return s


@pytest.mark.parametrize("keeper", ["first", "last", "delete_last", "absent", "alternating"])
def test_dp_gc_long_chains_lane_form_and_wave_form(dp, keeper):
    for n in (63, 64, 65, 300):
        s = chain_store(n, keeper)
        t = run_calls(dp, W.clone(s), [("gc", b"", b"", 10 * n + 5)], (0, 1, 4, 63, 64, 65, 300, 301))
        kept = [v.value for v in t.versions[b"hot"]]
        assert kept == ([b"above"] if keeper in ("absent", "delete_last") else [b"above", b"p%d" % (n - 1 if keeper == "last" else 0)])
        assert b"z" not in t.versions and t.versions[b"a"] == s.versions[b"a"]
        run_calls(dp, W.clone(s), [("gc", b"", b"", 10 * (n // 2)), ("gc", b"hot", b"hot\x00", 10), ("gc", b"hot", b"hot", U64)], (0, 4, 64))


def test_dp_ranges(dp):
    s = R.Store()
    for k in (b"4", b"4\x00", b"5", b"k" * 300, b"q"):
        s.put(k, b"v", 1, 2)
    s.prewrite([(R.OP_PUT, b"1", b"v"), (R.OP_PUT, b"4\x00", b"v"), (R.OP_PUT, b"zz", b"v")], b"1", 9)  # lock-only keys first and last
    ranges = [(b"", b""), (b"", b"5"), (b"4", b""), (b"5", b"5"), (b"4", b"4\x00"), (b"4\x00", b"5"), (b"41", b"42"), (b"6", b"j"), (b"9", b"2"), (b"1", b"zz"),
              (b"1", b"zz\x00"), (b"0", b"1"), (b"k" * 299, b"k" * 301)]
    lines = store_lines(s) + ["R %s %s" % (HEX(a), HEX(b)) for a, b in ranges]
    out = dp(lines)
    keys, vkeys, lkeys = s.keys(), [k for k, _ in entries(s)], sorted(s.locks)
    for (a, b), line in zip(ranges, out[1:]):
        u0, u1, e0, e1, l0, l1 = [int(x) for x in line.split()[1:]]
        assert keys[u0:u1] == MM.in_range(keys, a, b) and vkeys[e0:e1] == MM.in_range(vkeys, a, b) and lkeys[l0:l1] == MM.in_range(lkeys, a, b), (a, b)
    for a, b in ranges:
        run_calls(dp, W.clone(s), [("scan_lock", a, b, 9), ("delete_range", a, b)])
        run_calls(dp, W.clone(s), [("resolve", a, b, {9: 11}), ("gc", a, b, 9), ("gc", a, b, 8)])


# ------------------------------------------------------------------------------------------------ the C-ABI
NEW_SYMBOLS = ("tsq_mvcc_scan_lock", "tsq_mvcc_scan_lock_fetch", "tsq_mvcc_resolve_lock", "tsq_mvcc_gc", "tsq_mvcc_delete_range")


def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in abi.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    assert "#define TSQ_ABI_VERSION 10" in hdr and abi.TSQ_ABI_VERSION == 10 and lib.tsq_abi_version() == 10
    assert sorted(set(re.findall(r"\b(tsq_[a-z0-9_]+)\s*\(", hdr)) - {"tsq_status"}) == sorted(abi.SIGNATURES.keys())
    assert re.search(r"TSQ_KNOB_COUNT = 48\b", hdr)  # no new knob
    assert "EMPTY END DELETES NOTHING" in hdr and "*next = NULL" in hdr  # the two pinned departures


def test_struct_sizes_equal_what_gcc_computes_for_the_header(tmp_path):
    import ctypes as C
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", sizeof(tsq_mvcc_lock_scan), '
                   'sizeof(tsq_mvcc_maint_result), offsetof(tsq_mvcc_maint_result, first_error), offsetof(tsq_mvcc_maint_result, mark_ms));return 0;}\n'
                   % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.MvccLockScan), C.sizeof(abi.MvccMaintResult), abi.MvccMaintResult.first_error.offset, abi.MvccMaintResult.mark_ms.offset]
    for cls, name in ((abi.MvccLockScan, "tsq_mvcc_lock_scan"), (abi.MvccMaintResult, "tsq_mvcc_maint_result")):
        body = re.search(r"typedef struct %s \{(.*?)\}" % name, open(os.path.join(ROOT, "include", "tsq.h")).read(), re.S).group(1)
        assert [f for f, _ in cls._fields_] == re.findall(r"(\w+);", body)
