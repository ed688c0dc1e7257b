"""CPU: the model of the MVCC read side (tests/mvcc_ref.py) against the reference's own vectors (tests/golden/mvcc_cases.json), the
forward scan against the reverse scan, the host build of tsq_mvcc_dp.h (sanitized, a stand-alone program) against the model, and
the new part of the C-ABI."""
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import mvcc_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = lambda s: s.encode("latin-1")


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "mvcc_cases.json")))["cases"]


def play(case, on_read):
    """runs a golden case's operations on a model store; on_read(store, step) at every read step"""
    s = R.Store()
    for st in case["steps"]:
        op = st["op"]
        if op == "put":
            s.put(L1(st["key"]), L1(st["value"]), st["start_ts"], st["commit_ts"])
        elif op == "delete":
            s.delete(L1(st["key"]), st["start_ts"], st["commit_ts"])
        elif op == "prewrite":
            s.prewrite([(R.OP_NAMES[m[0]], L1(m[1]), L1(m[2])) for m in st["mutations"]], L1(st["primary"]), st["start_ts"], st["ttl"])
        elif op == "commit":
            s.commit([L1(k) for k in st["keys"]], st["start_ts"], st["commit_ts"])
        else:
            on_read(s, st)


def read_step_ranges(st):
    """a golden read step as (ranges, ts, desc, limit) of the range read"""
    if st["op"] == "get":
        return [(L1(st["key"]), None)], st["ts"], False, None
    return [(L1(st["start"]), L1(st["end"]))], st["ts"], st["op"] == "reverse_scan", st["limit"]


def step_expectation(st):
    """-> ("err",) or ("ok", pairs)"""
    if st["op"] == "get":
        if st["err"]:
            return ("err",)
        return ("ok", [] if st["expect"] is None else [(L1(st["key"]), L1(st["expect"]))])
    return ("ok", [(L1(k), L1(v)) for k, v in st["expect"]])


@pytest.mark.parametrize("case", golden(), ids=lambda c: c["name"])
def test_model_reproduces_the_references_vectors(case):
    reads = [0]

    def on_read(s, st):
        reads[0] += 1
        want = step_expectation(st)
        if st["op"] == "get":
            if want[0] == "err":
                with pytest.raises(R.ErrLocked):
                    s.get(L1(st["key"]), st["ts"])
            else:
                got = s.get(L1(st["key"]), st["ts"])
                assert ([] if got is None else [(L1(st["key"]), got)]) == want[1], st["line"]
        else:
            f = s.reverse_scan if st["op"] == "reverse_scan" else s.scan
            got = f(L1(st["start"]), L1(st["end"]), st["limit"], st["ts"])
            assert [(k, v) for k, v, e in got if e is None] == want[1] and all(e is None for _, _, e in got), st["line"]
        # ... and through the range read the GPU tests compare against
        ranges, ts, desc, limit = read_step_ranges(st)
        if want[0] == "err":
            with pytest.raises(R.ErrLocked):
                R.read_ranges(s, ranges, ts, desc, limit)
        else:
            assert R.read_ranges(s, ranges, ts, desc, limit)[0] == want[1], st["line"]
    play(case, on_read)
    assert reads[0] > 0


def test_the_golden_file_holds_every_vector_of_the_six_tests():
    n = {c["name"]: sum(1 for st in c["steps"] if st["op"] in ("get", "scan", "reverse_scan")) for c in golden()}
    # TestScan / TestReverseScan: checkV10 (12 lines) x 4 stages, checkV20 (6) x 3, checkV30 (3) x 2, checkV40 (2)
    assert n == {"TestGet": 4, "TestGetWithLock": 4, "TestDelete": 6, "TestCleanupRollback": 2, "TestReverseScan": 74, "TestScan": 74}


def test_lock_error_fields_and_the_encoded_key():
    s = R.Store()
    s.put(b"secondary", b"s-0", 1, 2)
    s.prewrite([(R.OP_PUT, b"primary", b"p-5"), (R.OP_PUT, b"secondary", b"s-5")], b"primary", 5, ttl=9)
    with pytest.raises(R.ErrLocked) as e:
        s.get(b"secondary", 8)
    # EncodeBytes("secondary"): "secondar" 0xFF, "y" + 7 zero bytes, 0xF8; EncodeUintDesc(lockVer) = 8 zero bytes
    assert e.value.fields() == (b"secondar\xffy" + b"\x00" * 7 + b"\xf8" + b"\x00" * 8, b"primary", 5, 9, R.OP_PUT)


def test_forward_and_reverse_scans_yield_the_same_set_per_range():
    rng = np.random.default_rng(11)
    compared = locked = 0
    for it in range(60):
        s = R.random_store(rng, int(rng.integers(1, 60)), "prefix" if it % 3 else "record")
        for ts in R.read_timestamps(s, rng, 4):
            for start, end in R.random_ranges(s, rng, 5):
                if end is None:
                    continue
                f, r = s.scan(start, end, R.NO_LIMIT, ts), s.reverse_scan(start, end, R.NO_LIMIT, ts)
                assert [(k, v, e is not None) for k, v, e in f] == [(k, v, e is not None) for k, v, e in reversed(r)]
                compared += len(f)
                locked += sum(1 for _, _, e in f if e is not None)
    assert compared > 2000 and locked > 20


# ------------------------------------------------------------------------------------------------ the host build of tsq_mvcc_dp.h
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("mvcc_dp") / "mvcc_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "mvcc_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        return res.stdout.split("\n")
    return run


HEX = lambda b: b.hex() if b else "-"


def store_lines(flat):
    ko, vo, lo, po = flat["key_offsets"], flat["value_offsets"], flat["lock_key_offsets"], flat["lock_primary_offsets"]
    kb, lb, pb = flat["keys"].tobytes(), flat["lock_keys"].tobytes(), flat["lock_primaries"].tobytes()
    n, nl = len(ko) - 1, len(lo) - 1
    out = ["S %d %d" % (n, nl)]
    for i in range(n):
        out.append("%s %d %d %d" % (HEX(kb[ko[i]:ko[i + 1]]), int(flat["commit_ts"][i]), int(flat["types"][i]), vo[i + 1] - vo[i]))
    for j in range(nl):
        out.append("%s %d %d %s" % (HEX(lb[lo[j]:lo[j + 1]]), int(flat["lock_start_ts"][j]), int(flat["lock_ops"][j]), HEX(pb[po[j]:po[j + 1]])))
    return out


def query_lines(ranges, ts, desc, limit, chain):
    out = ["Q %d %d %d %d %d" % (ts, 1 if desc else 0, -1 if limit is None else limit, chain, len(ranges))]
    for start, end in ranges:
        out.append("%s %s %d" % (HEX(start), HEX(end or b""), 1 if end is None else 0))
    return out


def entry_pairs(flat):
    ko, vo = flat["key_offsets"], flat["value_offsets"]
    kb, vb = flat["keys"].tobytes(), flat["values"].tobytes()
    return [(kb[ko[i]:ko[i + 1]], vb[vo[i]:vo[i + 1]]) for i in range(len(ko) - 1)]


def model_answer(s, ranges, ts, desc, limit):
    try:
        pairs, counts = R.read_ranges(s, ranges, ts, desc, limit)
        return ("ok", pairs, counts)
    except R.ErrLocked as e:
        return ("locked", e.RawKey)


def check_queries(dp, s, queries):
    """queries: [(ranges, ts, desc, limit, chain)] — one program run, every answer against the model"""
    flat = s.flat()
    lines = store_lines(flat)
    for q in queries:
        lines += query_lines(*q)
    out = dp(lines)
    assert out[0] == "U %d" % len(s.keys())
    ep = entry_pairs(flat)
    lock_keys = sorted(s.locks)
    kinds = {"ok": 0, "locked": 0}
    for i, (ranges, ts, desc, limit, chain) in enumerate(queries):
        head, sel, counts = out[1 + 3 * i].split(), out[2 + 3 * i].split(), out[3 + 3 * i].split()
        want = model_answer(s, ranges, ts, desc, limit)
        kinds[want[0]] += 1
        if want[0] == "locked":
            assert head[1] == "17" and lock_keys[int(head[3])] == want[1], (ranges, ts, desc, limit)
        else:
            assert head[1] == "0" and int(head[2]) == len(want[1])
            assert [ep[int(x)] for x in sel] == want[1], (ranges, ts, desc, limit)
            assert [int(x) for x in counts] == want[2]
    return kinds


def test_dp_header_against_the_model_on_random_stores_sanitized(dp):
    rng = np.random.default_rng(5)
    kinds = {"ok": 0, "locked": 0}
    for it in range(40):
        s = R.random_store(rng, int(rng.choice([1, 2, 7, 63, 64, 65, 130])), "prefix" if it % 4 else "record", max_chain=int(rng.choice([1, 5, 9])))
        qs = []
        for ts in R.read_timestamps(s, rng, 3):
            ranges = R.random_ranges(s, rng, int(rng.integers(0, 6)))
            total = len(model_answer(s, ranges, ts, False, None)[1]) if model_answer(s, ranges, ts, False, None)[0] == "ok" else 3
            for limit in (None, 0, 1, max(total - 1, 0), total, total + 1):
                for desc in (False, True):
                    rr = list(reversed(ranges)) if desc else ranges
                    qs.append((rr, ts, desc, limit, int(rng.choice([0, 1, 2, 3, 64]))))
        got = check_queries(dp, s, qs)
        for k in kinds:
            kinds[k] += got[k]
    assert kinds["ok"] > 1000 and kinds["locked"] > 100


def test_dp_long_chains_lane_form_and_wave_form(dp):
    s = R.Store()
    n = 700
    s.versions[b"hot"] = [R.Value(R.PUT, 2 * c, 2 * c + 1, b"h%d" % c) for c in range(n, 0, -1)]  # commitTS 2n + 1 .. 3
    s.versions[b"roll"] = [R.Value(R.ROLLBACK, c, c, b"") for c in range(1400, 1100, -1)] + [R.Value(R.DELETE, 90, 91, b""), R.Value(R.PUT, 10, 11, b"old")]
    s.versions[b"rollput"] = [R.Value(R.ROLLBACK, c, c, b"") for c in range(1400, 1100, -1)] + [R.Value(R.PUT, 10, 11, b"kept")]
    s.versions[b"a"] = [R.Value(R.PUT, 1, 2, b"a")]
    qs = []
    for chain in (0, 1, 64, 299, 300, 301, 302, 303, 699, 700, 701):
        for ts in (0, 2, 3, 4, 11, 91, 1100, 1101, 1250, 1400, 1401, 2 * n, 2 * n + 1, 2 * n + 2, R.U64_MAX):
            qs.append(([(b"", b"")], ts, False, None, chain))
            qs.append(([(b"", b"")], ts, True, 2, chain))
    assert check_queries(dp, s, qs)["ok"] == len(qs)


def test_dp_create_checks(dp):
    A, B = b"A", b"B"
    bits = lambda *a, **k: int(dp(store_lines(R.flat_arrays(*a, **k)))[0].split()[1])
    no_locks = ([], [], [], [], [])
    assert dp(store_lines(R.flat_arrays([A, A, B], [9, 5, 5], [0, 0, 0], [0, 1, 2], [b"x", b"", b""], *no_locks)))[0] == "U 2"
    assert bits([B, A], [5, 5], [0, 0], [0, 0], [b"x", b"y"], *no_locks) == 4  # keys not ascending
    assert bits([A, B, A], [5, 5, 4], [0, 0, 0], [0, 0, 0], [b"x", b"y", b"z"], *no_locks) == 4  # ... a key that comes back
    assert bits([A, A], [5, 5], [0, 0], [0, 0], [b"x", b"y"], *no_locks) == 8  # equal commitTS
    assert bits([A, A], [5, 6], [0, 0], [0, 0], [b"x", b"y"], *no_locks) == 8  # ascending commitTS
    assert dp(store_lines(R.flat_arrays([A, A], [1 << 63, (1 << 63) - 1], [0, 0], [0, 0], [b"x", b"y"], *no_locks)))[0] == "U 1"  # unsigned order
    assert bits([A, A], [(1 << 63) - 1, 1 << 63], [0, 0], [0, 0], [b"x", b"y"], *no_locks) == 8
    assert bits([b"", A], [5, 5], [0, 0], [0, 0], [b"x", b"y"], *no_locks) == 2  # empty key
    assert bits([A], [5], [0], [0], [b""], *no_locks) == 16  # a put with an empty value
    assert bits([A], [5], [0], [3], [b""], *no_locks) == 32  # type out of range
    assert bits([A], [5], [0], [0], [b"x"], [B, A], [1, 1], [0, 0], [0, 0], [A, A]) == 64  # lock keys not ascending
    assert bits([A], [5], [0], [0], [b"x"], [B, B], [1, 1], [0, 0], [0, 0], [A, A]) == 128  # two locks on one key
    assert bits([A], [5], [0], [0], [b"x"], [B], [1], [0], [4], [A]) == 32  # op out of range
    assert bits([A], [5], [0], [0], [b"x"], [b""], [1], [0], [0], [A]) == 2  # empty lock key


# ------------------------------------------------------------------------------------------------ the C-ABI
def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("tsq_mvcc_create", "tsq_mvcc_scan", "tsq_mvcc_fetch", "tsq_mvcc_locked", "tsq_mvcc_stats", "tsq_mvcc_cancel", "tsq_mvcc_destroy"):
        assert hasattr(lib, name) and name in abi.SIGNATURES
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    assert re.search(r"TSQ_ERR_LOCKED = 17\b", hdr) and "#define TSQ_ABI_VERSION 10" in hdr
    assert abi.ERR_LOCKED == 17 and abi.STATUS_NAMES[17] == "LOCKED" and abi.TSQ_ABI_VERSION == 10
    assert sorted(set(re.findall(r"\b(tsq_[a-z0-9_]+)\s*\(", hdr)) - {"tsq_status"}) == sorted(abi.SIGNATURES.keys())
    for name, val in (("PUT", 0), ("DELETE", 1), ("ROLLBACK", 2), ("OP_PUT", 0), ("OP_DEL", 1), ("OP_LOCK", 2), ("OP_ROLLBACK", 3)):
        assert re.search(r"#define TSQ_MVCC_%s %d\b" % (name, val), hdr) and getattr(abi, "MVCC_" + name) == val
    assert re.search(r"#define TSQ_KNOB_MVCC_WAVE_CHAIN TSQ_KNOB_XCD_ATOMICS\b", hdr) and re.search(r"TSQ_KNOB_XCD_ATOMICS = 30,", hdr) and abi.KNOB_MVCC_WAVE_CHAIN == 30 and re.search(r"TSQ_KNOB_COUNT = 48\b", hdr)
    assert (R.PUT, R.DELETE, R.ROLLBACK, R.OP_PUT, R.OP_DEL, R.OP_LOCK, R.OP_ROLLBACK) == (0, 1, 2, 0, 1, 2, 3)


def test_struct_sizes_equal_what_gcc_computes_for_the_header(tmp_path):
    import ctypes as C
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", sizeof(tsq_mvcc_data), sizeof(tsq_mvcc_result), '
                   'offsetof(tsq_mvcc_data, n_locks), offsetof(tsq_mvcc_data, data_flags));return 0;}\n' % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.MvccData), C.sizeof(abi.MvccResult), abi.MvccData.n_locks.offset, abi.MvccData.data_flags.offset]


def test_python_layer_encodes_the_lock_key_like_the_model():
    from tinysql_amd import mvcc
    for key in (b"", b"a", b"12345678", b"secondary", b"\x00\xff" * 9):
        assert mvcc.mvccEncode(key, R.U64_MAX) == R.mvcc_encode(key, R.LOCK_VER) and mvcc.mvccEncode(key, 7) == R.mvcc_encode(key, 7)
    assert R.prefix_next(b"a\xff") == b"b\x00" and R.prefix_next(b"\xff\xff") == b"\xff\xff\x00" and R.prefix_next(b"ab") == b"ac"
