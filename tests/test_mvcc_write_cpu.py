"""CPU: the model of the MVCC writes (tests/mvcc_write_ref.py) against the write steps of the reference's own tests
(tests/golden/mvcc_write_cases.json), the host build of tsq_mvcc_write_dp.h (sanitized, a stand-alone program) against the model —
verdicts, and the plan of every key applied to the store's arrays — in the lane and the wave form of the chain walk, and the new part
of the C-ABI."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mvcc_ref as R
from tests import mvcc_write_ref as W
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = lambda s: s.encode("latin-1")
HEX = lambda b: b.hex() if b else "-"


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "mvcc_write_cases.json")))["cases"]


def step_call(st):
    """a golden write step as the call tuple of mvcc_write_ref.apply_call"""
    if st["op"] == "prewrite":
        return ("prewrite", [(R.OP_NAMES[m[0]], L1(m[1]), L1(m[2])) for m in st["mutations"]], L1(st["primary"]), st["start_ts"], st["ttl"])
    if st["op"] == "commit":
        return ("commit", [L1(k) for k in st["keys"]], st["start_ts"], st["commit_ts"])
    return ("rollback", [L1(k) for k in st["keys"]], st["start_ts"])


def check_step_details(s_before, st, call, verdicts):
    """the fields the golden file records beside the verdict codes"""
    if "lock" in st:
        lk = sorted(s_before.locks)[verdicts[0][1]]
        l = s_before.locks[lk]
        assert (lk, l.primary, l.start_ts, l.ttl, l.op) == (L1(st["lock"]["key"]), L1(st["lock"]["primary"]), st["lock"]["start_ts"], st["lock"]["ttl"],
                                                         R.OP_NAMES[st["lock"]["op"]]), st["line"]
    for v, c in zip(verdicts, st.get("conflicts", [])):
        if c is not None:
            assert (call[3], v[1], v[2]) == (c["start_ts"], c["conflict_ts"], c["conflict_commit_ts"]), st["line"]
    for v, c in zip(verdicts, st.get("already_committed", [])):
        assert v[1] == c, st["line"]


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_model_reproduces_the_references_write_steps(case):
    s = R.Store()
    writes = 0
    for st in case["steps"]:
        if st["op"] == "noop":
            continue
        if st["op"] == "get":
            if st["err"]:
                with pytest.raises(R.ErrLocked):
                    s.get(L1(st["key"]), st["ts"])
            else:
                assert s.get(L1(st["key"]), st["ts"]) == (None if st["expect"] is None else L1(st["expect"])), st["line"]
            continue
        call = step_call(st)
        before = W.clone(s)
        verdicts, applied = W.apply_call(s, call)
        assert [v[0] for v in verdicts] == [W.NAMES[x] for x in st["verdicts"]], st["line"]
        assert applied == all(x in ("ok", "noop") for x in st["verdicts"]) and applied == (st["asserts"] == "ok"), st["line"]
        if not applied:  # any error writes nothing
            assert s.versions == before.versions and s.locks == before.locks, st["line"]
        check_step_details(before, st, call, verdicts)
        writes += 1
    assert writes >= 4


def test_the_golden_file_holds_the_five_tests():
    n = {c["name"]: sum(1 for st in c["steps"] if st["op"] in ("prewrite", "commit", "rollback")) for c in golden()}
    assert n == {"TestCommitConflict": 8, "TestRollbackAndWriteConflict": 6, "TestCleanupRollback": 5, "TestGetWithLock": 5, "TestDelete": 4}
    noop = [st for c in golden() for st in c["steps"] if st["op"] == "noop"]
    assert len(noop) == 1 and noop[0]["line"] == ":538"


def test_model_semantics_every_verdict_any_error_nothing_first_error():
    s = R.Store()
    s.put(b"b", b"b1", 5, 10)
    s.prewrite([(R.OP_PUT, b"c", b"c7")], b"c", 7)
    before = W.clone(s)
    verdicts, applied = W.prewrite(s, [(R.OP_PUT, b"a", b"x"), (R.OP_PUT, b"b", b"x"), (R.OP_PUT, b"c", b"x"), (R.OP_PUT, b"d", b"x")], b"a", 9)
    assert verdicts == [(W.OK, 0, 0), (W.CONFLICT, 5, 10), (W.LOCKED, 0, 0), (W.OK, 0, 0)] and not applied
    assert s.versions == before.versions and s.locks == before.locks
    # a key without versions conflicts exactly at startTS 0, with both fields 0
    assert W.prewrite_verdict(s, b"zz", 0) == (W.CONFLICT, 0, 0) and W.prewrite_verdict(s, b"zz", 1) == (W.OK, 0, 0)
    # unsigned: a commitTS of 2^63 is newer than a startTS of 2^63 - 1
    s.put(b"u", b"u", 1 << 62, 1 << 63)
    assert W.prewrite_verdict(s, b"u", (1 << 63) - 1)[0] == W.CONFLICT and W.prewrite_verdict(s, b"u", (1 << 63) + 1)[0] == W.OK
    # Commit: every key a verdict, first_error the reference's (the first failing key in key order)
    keys = [b"a", b"b", b"c", b"q"]
    verdicts, applied = W.commit(s, keys, 7, 8)
    assert [v[0] for v in verdicts] == [W.TXN_NOT_FOUND, W.TXN_NOT_FOUND, W.OK, W.TXN_NOT_FOUND] and not applied and b"c" in s.locks
    assert W.first_error(verdicts, keys) == 0
    verdicts, applied = W.commit(s, [b"b", b"c"], 5, 10)  # b is committed by 5: a no-op; c's lock is another transaction's
    assert [v[0] for v in verdicts] == [W.NOOP, W.TXN_NOT_FOUND] and W.first_error(verdicts, [b"b", b"c"]) == 1
    # Rollback: already committed carries the commitTS; the rollback beside a foreign lock leaves the lock
    assert W.rollback(s, [b"b"], 5) == ([(W.ALREADY_COMMITTED, 10, 0)], False)
    assert W.rollback(s, [b"c"], 3) == ([(W.OK, 0, 0)], True) and s.locks[b"c"].start_ts == 7 and s.versions[b"c"] == [R.Value(R.ROLLBACK, 3, 3, b"")]
    assert W.rollback(s, [b"c"], 3) == ([(W.NOOP, 0, 0)], True)


def test_model_agrees_with_the_host_model_of_mvcc_ref_where_that_one_succeeds():
    """mvcc_ref.Store.prewrite / commit / rollback raise at the first error and have written what came before it; on calls without an
    error both models must leave the same store"""
    rng = np.random.default_rng(3)
    agreed = 0
    for it in range(30):
        s = W.writable_random_store(rng, int(rng.integers(0, 30)))
        for _ in range(30):
            call = W.random_call(s, rng, [20, 1000, (1 << 63) + 3], [b"fresh%d" % i for i in range(4)])
            a, b = W.clone(s), W.clone(s)
            verdicts, applied = W.apply_call(a, call)
            if not applied:
                continue
            getattr(b, call[0])(*call[1:])
            assert a.versions == b.versions and a.locks == b.locks, call
            s = a
            agreed += 1
    assert agreed > 200


# ------------------------------------------------------------------------------------------------ the host build of tsq_mvcc_write_dp.h
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mvcc_write_dp") / "mvcc_write_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "mvcc_write_dp_main.cpp"), "-o", str(exe)], check=True)

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


def sorted_request(call):
    """the request as the C-ABI takes it: keys strictly ascending (a key named twice: the last one wins) -> (kind, [(key, op, value)],
    start_ts, commit_ts, caller index per sorted key)"""
    if call[0] == "prewrite":
        last = {}
        for i, (op, key, value) in enumerate(call[1]):
            last[key] = i
        order = sorted(last.values(), key=lambda i: call[1][i][1])
        return 0, [(call[1][i][1], call[1][i][0], call[1][i][2]) for i in order], call[3], 0, order
    order = sorted(range(len(call[1])), key=lambda i: call[1][i])
    return (1 if call[0] == "commit" else 2), [(call[1][i], 0, b"") for i in order], call[2], (call[3] if call[0] == "commit" else 0), order


def call_lines(call, chain):
    kind, rows, start_ts, commit_ts, _ = sorted_request(call)
    return ["W %d %d %d %d %d" % (kind, start_ts, commit_ts, chain, len(rows))] + ["%s %d %d" % (HEX(k), op, len(v)) for k, op, v in rows]


def apply_plan(s, call, plans):
    """the plan of every key applied to the store's arrays the way tsq_mvcc_write.hip's apply does: a new version goes before the
    entry at its version index, a replaced entry goes; a new lock goes before the lock at its lock index, a dropped lock goes"""
    kind, rows, start_ts, commit_ts, _ = sorted_request(call)
    lock_keys = sorted(s.locks)
    versions = [(p, 1, key, v) for p, (key, v) in enumerate((key, v) for key in sorted(s.versions) for v in s.versions[key])]
    locks = [(j, 1, key, s.locks[key]) for j, key in enumerate(lock_keys)]
    for i, ((key, op, value), pl) in enumerate(zip(rows, plans)):
        verdict, info0, info1, flags, vtype, vsrc, vpos, lpos = pl
        if flags & 2:
            versions = [e for e in versions if not (e[0] == vpos and e[1] == 1)]
        if flags & 1:
            val = s.locks[lock_keys[vsrc]].value if vsrc >= 0 else b""
            versions.append((vpos, 0, key, R.Value(vtype, start_ts, commit_ts if kind == 1 else start_ts, val)))
        if flags & 8:
            locks = [e for e in locks if not (e[0] == lpos and e[1] == 1)]
        if flags & 4:
            locks.append((lpos, 0, key, R.Lock(start_ts, call[2], value, op, call[4])))
    out = R.Store()
    for _, _, key, v in sorted(versions, key=lambda e: (e[0], e[1])):  # (stable: new entries at one index keep the request's order)
        out.versions.setdefault(key, []).append(v)
    for _, _, key, l in sorted(locks, key=lambda e: (e[0], e[1])):
        assert key not in out.locks
        out.locks[key] = l
    return out


def run_history(dp, s, calls, chains):
    """one program run per store state would be slow: the store is sent again only after a call that changed it.  Every call is asked
    with every chain threshold; returns the kinds met."""
    kinds = set()
    for call in calls:
        lines = store_lines(s)
        for chain in chains:
            lines += call_lines(call, chain)
        out = dp(lines)
        assert out[0] == "U %d" % len(s.keys())
        model = W.clone(s)
        verdicts, applied = W.apply_call(model, call)
        kinds |= W.call_kinds(call, verdicts)
        kind, rows, start_ts, commit_ts, order = sorted_request(call)
        want = [verdicts[i] for i in order]
        q, at = len(rows), 1
        for chain in chains:
            head = out[at].split()
            plans = [tuple(int(x) for x in out[at + 1 + i].split()) for i in range(q)]
            at += 1 + q
            assert [p[:3] for p in plans] == want, (call, chain)
            bad = [i for i, v in enumerate(want) if v[0] >= W.LOCKED]
            assert head == ["W", str(len(bad)), str(bad[0] if bad else -1)]
            if applied:
                got = apply_plan(s, call, plans)
                assert got.versions == model.versions and got.locks == model.locks, (call, chain)
                for key, vs in got.versions.items():  # the arrays stay a store: descending commitTS inside every key
                    assert all(a.commit_ts > b.commit_ts for a, b in zip(vs, vs[1:]))
        s = model
    return s, kinds


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_dp_header_on_the_golden_cases_sanitized(dp, case):
    calls = [step_call(st) for st in case["steps"] if st["op"] in ("prewrite", "commit", "rollback")]
    run_history(dp, R.Store(), calls, (0, 1))


def test_dp_header_against_the_model_on_random_histories_sanitized(dp):
    rng = np.random.default_rng(7)
    kinds = set()
    for it, n_keys in enumerate([0, 1, 2, 7, 63, 64, 65, 130]):
        s = W.writable_random_store(rng, n_keys, "prefix" if it % 3 else "record", max_chain=int(rng.choice([1, 5, 9])))
        fresh = [b"A", b"\xff\xff", b"AAB\x00n"] + [b"f%d" % i for i in range(3)]
        txns = [30, 1001, (1 << 63) + 5]
        calls = []
        for _ in range(30):
            calls.append(W.random_call(s, rng, txns, fresh))
        s2 = s
        for call in calls:  # (random_call looks at the store as it is then)
            s2, k = run_history(dp, s2, [call], (0, 1, 3))
            kinds |= k
    assert kinds == W.ALL_KINDS, W.ALL_KINDS - kinds


def test_dp_long_chains_lane_form_and_wave_form(dp):
    for n in (63, 64, 65, 300):
        s = R.Store()
        # the wanted start_ts last in the chain; commitTS descending; `other` has it nowhere
        s.versions[b"hot"] = [R.Value(R.PUT, 10 * c, 10 * c + 1, b"h") for c in range(n, 1, -1)] + [R.Value(R.PUT, 7, 8, b"first")]
        s.versions[b"rolled"] = [R.Value(R.PUT, 10 * c, 10 * c + 1, b"h") for c in range(n, 1, -1)] + [R.Value(R.ROLLBACK, 7, 7, b"")]
        s.versions[b"other"] = [R.Value(R.PUT, 10 * c, 10 * c + 1, b"h") for c in range(n, 0, -1)]
        keys = [b"hot", b"other", b"rolled"]
        calls = [("commit", keys, 7, 9), ("rollback", [b"hot"], 7), ("rollback", [b"other", b"rolled"], 7), ("rollback", [b"other"], 10 * n + 5),
                 ("commit", [b"other"], 20, 21), ("rollback", [b"other"], 15)]
        _, kinds = run_history(dp, s, calls, (0, 1, 63, 64, 65, 300, 301))
        assert kinds == {"txn_not_found", "already_committed", "noop_commit", "noop_rollback"}


def test_dp_request_checks(dp):
    s = R.Store()
    s.put(b"b", b"v", 1, 2)
    def bits(lines):  # the error bits; 0: the request passed and got its verdicts
        head = dp(store_lines(s) + lines)[1].split()
        return int(head[1]) if head[0] == "E" else 0
    assert bits(["W 0 5 0 0 2", "61 0 1", "62 0 1"]) == 0
    assert bits(["W 0 5 0 0 2", "62 0 1", "61 0 1"]) == 4  # not ascending
    assert bits(["W 1 5 6 0 2", "61 0 0", "61 0 0"]) == 4  # a key twice
    assert bits(["W 0 5 0 0 2", "61 0 1", "6100 0 1"]) == 0  # a key that extends its neighbour
    assert bits(["W 2 5 0 0 1", "- 0 0"]) == 2  # empty key
    assert bits(["W 0 5 0 0 1", "61 3 1"]) == 8  # Op_Rollback is no prewrite op
    assert bits(["W 0 5 0 0 1", "61 0 0"]) == 16  # a put with an empty value
    assert bits(["W 0 5 0 0 2", "61 1 0", "62 2 0"]) == 0  # Del and Lock come without one
    assert bits(["W 1 5 6 0 1", "61 3 0"]) == 0  # Commit reads no ops


# ------------------------------------------------------------------------------------------------ the C-ABI
NEW_SYMBOLS = ("tsq_mvcc_create_rw", "tsq_mvcc_prewrite", "tsq_mvcc_commit", "tsq_mvcc_rollback", "tsq_mvcc_lock_at", "tsq_mvcc_sizes", "tsq_mvcc_export")


def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = _lib.load()
    for name in NEW_SYMBOLS:
        assert hasattr(lib, name) and name in abi.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    assert "#define TSQ_ABI_VERSION 10" in hdr and abi.TSQ_ABI_VERSION == 10 and lib.tsq_abi_version() == 10
    assert sorted(set(re.findall(r"\b(tsq_[a-z0-9_]+)\s*\(", hdr)) - {"tsq_status"}) == sorted(abi.SIGNATURES.keys())
    for name, val in (("OK", 0), ("NOOP", 1), ("LOCKED", 2), ("CONFLICT", 3), ("TXN_NOT_FOUND", 4), ("ALREADY_COMMITTED", 5)):
        assert re.search(r"#define TSQ_MVCC_V_%s %d\b" % (name, val), hdr) and getattr(abi, "MVCC_V_" + name) == val and getattr(W, name) == val
    assert re.search(r"TSQ_KNOB_COUNT = 48\b", hdr)  # no new knob


def test_struct_sizes_equal_what_gcc_computes_for_the_header(tmp_path):
    import ctypes as C
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu %%zu %%zu %%zu\\n", sizeof(tsq_mvcc_write_req), '
                   'sizeof(tsq_mvcc_write_result), sizeof(tsq_mvcc_store_sizes), sizeof(tsq_mvcc_arrays), offsetof(tsq_mvcc_write_req, start_ts), '
                   'offsetof(tsq_mvcc_write_req, flags), offsetof(tsq_mvcc_write_result, kernel_ms));return 0;}\n' % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.MvccWriteReq), C.sizeof(abi.MvccWriteResult), C.sizeof(abi.MvccStoreSizes), C.sizeof(abi.MvccArrays),
                   abi.MvccWriteReq.start_ts.offset, abi.MvccWriteReq.flags.offset, abi.MvccWriteResult.kernel_ms.offset]
    assert [f for f, _ in abi.MvccArrays._fields_] == re.findall(r"\*\s*(\w+);", re.search(r"typedef struct tsq_mvcc_arrays \{(.*?)\}", open(
        os.path.join(ROOT, "include", "tsq.h")).read(), re.S).group(1))
