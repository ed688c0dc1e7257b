"""CPU side of the duplicate-key checker (tsq_dupcheck_*, tsq_rows_equal).  (1) The sequential model (tests/dupcheck_ref.py) against
the reference's own REPLACE vectors (tests/golden/replace_cases.json, executor/write_test.go:376-446).  (2) The parallel form the GPU
computes (tests/dupcheck_form.py) against the model on random statements whose keys nearly all collide.  (3) The per-key and per-cell
code of the kernels (tinysql_amd/csrc/tsq_dupcheck_dp.h) built on the host as a stand-alone sanitized program.  (4) Header and binding of
the new entry points."""
import bisect
import json
import os
import struct
import subprocess

import numpy as np
import pytest

from tests import dupcheck_form as F
from tests import dupcheck_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
TYPES = {"i64": abi.I64, "f64": abi.F64, "bytes": abi.BYTES}


def same_rows(a, b):
    """rows / tables compared cell by cell by their printed form: a NaN equals itself here, -0.0 differs from 0.0"""
    return repr(a) == repr(b)


# ---------------------------------------------------------------- (1) the model and the reference's vectors
def golden_cases():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "replace_cases.json")))["cases"]


@pytest.mark.parametrize("case", golden_cases(), ids=lambda c: c["name"])
def test_model_gives_the_references_affected_rows_and_tables(case):
    shape = R.TableShape([TYPES[t] for t in case["col_types"]], case["pk_col"], case["uniques"])
    store = R.Store(shape, [(h, tuple(r)) for h, r in case["stored"]])
    base = max([h for h, _ in case["stored"]], default=0)
    for st in case["statements"]:
        rows = [tuple(r) for r in st["rows"]]
        stored = sorted(store.table().items())
        form = F.parallel_replace(shape, stored, rows, base)
        res = R.replace_stmt(shape, store, rows, base)
        base = res["rowid_base"]
        if st["affected"] is not None:
            assert res["affected"] == st["affected"], "line %d" % st["line"]
        assert form["affected"] == res["affected"] and same_rows(form["table"], store.table()), "line %d" % st["line"]
    if case["final"] is not None:
        assert sorted(store.table().values()) == sorted(tuple(r) for r in case["final"])


def test_the_ten_asserted_values_are_all_there():
    got = [st["affected"] for c in golden_cases() for st in c["statements"] if st["affected"] is not None]
    assert got == [1, 2, 1, 1, 1, 3, 1, 2, 7, 2]


# ---------------------------------------------------------------- (2) the parallel form against the model
def random_shape(rng):
    """(id-ish BIGINT, BIGINT, string, DOUBLE payload); PK handle or not; 0-3 unique indexes over the int / string columns (one of them
    two-column, one a prefix index)"""
    pk = 0 if rng.random() < 0.5 else None
    pool = [[(1, None)], [(2, None)], [(1, None), (2, None)], [(2, 2)]]
    k = int(rng.integers(0, 4))
    uniques = [pool[i] for i in rng.permutation(len(pool))[:k]]
    return R.TableShape([abi.I64, abi.I64, abi.BYTES, abi.F64], pk, uniques)


def random_rows(rng, n, dom, copy_from=()):
    """copy_from: rows that a third of the new rows repeat cell for cell (an earlier row of the statement or a stored row: the
    "unchanged" branch needs whole rows to be equal, which four random cells rarely are)"""
    words = [b"", b"a", b"ab", b"abc", b"abd", b"ab\0", b"b", b"ba", b"abcdefgh", b"abcdefghi", b"abcdefgi", b"c"]
    reals = [0.0, -0.0, 1.5, float("nan")]
    rows = []
    copy_from = list(copy_from)
    for _ in range(n):
        if (copy_from or rows) and rng.random() < 0.33:
            src = copy_from + rows
            rows.append(src[int(rng.integers(0, len(src)))])
            continue
        rows.append((int(rng.integers(0, dom)), None if rng.random() < 0.12 else int(rng.integers(0, dom)),
                     None if rng.random() < 0.12 else words[int(rng.integers(0, min(dom, len(words))))],
                     None if rng.random() < 0.1 else reals[int(rng.integers(0, 4))]))
    return rows


def random_store(rng, shape, dom):
    """a CONSISTENT store of 0-6 rows: random rows REPLACEd into an empty table"""
    store = R.Store(shape)
    res = R.replace_stmt(shape, store, random_rows(rng, int(rng.integers(0, 7)), dom), 0)
    return sorted(store.table().items()), res["rowid_base"]


def test_parallel_replace_equals_the_sequential_model_on_random_statements():
    rng = np.random.default_rng(20240607)
    unchanged = removed_batch = removed_store = 0
    for it in range(10000):
        shape = random_shape(rng)
        dom = int(rng.integers(2, 13))
        stored, base = random_store(rng, shape, dom)
        rows = random_rows(rng, int(rng.integers(0, 9)), dom, [r for _, r in stored])
        form = F.parallel_replace(shape, stored, rows, base)
        store = R.Store(shape, stored)
        res = R.replace_stmt(shape, store, rows, base)
        ctx = "statement %d: pk=%r uniques=%r stored=%r rows=%r" % (it, shape.pk_col, shape.uniques, stored, rows)
        assert form["added"] == res["added"], ctx
        assert form["handles"] == res["handles"] and form["put"] == res["put"], ctx
        assert form["removed_store"] == res["removed_store"] and form["n_removed_batch"] == res["n_removed_batch"], ctx
        assert form["affected"] == res["affected"] and form["rowid_base"] == res["rowid_base"], ctx
        assert same_rows(sorted(form["table"].items()), sorted(store.table().items())), ctx
        unchanged += res["added"].count(False)
        removed_batch += res["n_removed_batch"]
        removed_store += len(res["removed_store"])
    assert min(unchanged, removed_batch, removed_store) > 1000  # the statements did collide


def test_parallel_insert_equals_the_sequential_model_on_random_statements():
    rng = np.random.default_rng(7)
    kinds = {"ok": 0, "store": 0, "batch": 0}
    for it in range(4000):
        shape = random_shape(rng)
        dom = int(rng.integers(2, 40))
        stored, base = random_store(rng, shape, dom)
        rows = random_rows(rng, int(rng.integers(0, 6)), dom)
        form = F.parallel_insert(shape, stored, rows)
        ctx = "statement %d: pk=%r uniques=%r stored=%r rows=%r" % (it, shape.pk_col, shape.uniques, stored, rows)
        try:
            R.insert_stmt(shape, R.Store(shape, stored), rows, base)
            assert form is None, ctx
            kinds["ok"] += 1
        except R.KeyExists as e:
            assert form is not None and (form[0], form[1]) == (e.row, e.stream), ctx
            if form[2]:
                assert form[3] == e.dup_handle, ctx
                kinds["store"] += 1
            else:  # the entry of the FIRST row of the group; without a PK handle that row took rowid_base + its position + 1
                h = rows[form[4]][shape.pk_col] if shape.pk_col is not None else base + form[4] + 1
                assert h == e.dup_handle, ctx
                kinds["batch"] += 1
    assert min(kinds.values()) > 200, kinds


# ---------------------------------------------------------------- (3) the kernels' per-key / per-cell code, sanitized
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("dupcheck") / "dupcheck_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "dupcheck_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        return [[int(x) for x in ln.split()] for ln in res.stdout.splitlines()]
    return run


def hx(b):
    return b.hex() if b else "-"


def key_pool(rng):
    """keys of 0..70 bytes that share long prefixes: pairs that differ only in their last byte, only in length, and at every position
    around the 8-byte pieces"""
    base = bytes(rng.integers(0, 256, 70, dtype=np.uint8))
    keys = {b""}
    for n in range(0, 71):
        keys.add(base[:n])
        if n:
            keys.add(base[:n - 1] + bytes([(base[n - 1] + 1) & 255]))
            keys.add(base[:n - 1] + b"\0")
            keys.add(base[:n - 1] + b"\xff")
    return sorted(keys)


def test_key_search_and_compare_on_the_host_sanitized(dp):
    rng = np.random.default_rng(3)
    pool = key_pool(rng)
    for take in (0, 1, 2, 15, 16, 17, len(pool) // 2):
        store = sorted(pool[i] for i in rng.choice(len(pool), take, replace=False)) if take else []
        got = dp(["K %d %s" % (len(store), " ".join(hx(k) for k in store)), "P %d %s" % (len(pool), " ".join(hx(k) for k in pool))])
        for k, (find, lower) in zip(pool, got):
            lo = bisect.bisect_left(store, k)
            assert lower == lo and find == (lo if lo < len(store) and store[lo] == k else -1), (take, k)
    pairs = [(pool[i], pool[j]) for i, j in rng.integers(0, len(pool), (3000, 2))] + [(k, k) for k in pool[:80]]
    got = dp(["C %s %s" % (hx(a), hx(b)) for a, b in pairs])
    for (a, b), (c, e) in zip(pairs, got):
        assert c == (a > b) - (a < b) and e == (a == b), (a, b)


def test_cell_equality_on_the_host_sanitized(dp):
    bits = lambda x: struct.unpack("<Q", struct.pack("<d", x))[0]
    reals = [0.0, -0.0, 1.5, -1.5, float("inf"), float("nan"), 5e-324]
    got = dp(["D %x %x" % (bits(a), bits(b)) for a in reals for b in reals])
    want = [[int(R.datum_equal(a, b))] for a in reals for b in reals]
    assert got == want and want[reals.index(0.0) * len(reals) + reals.index(-0.0)] == [1] and want[5 * len(reals) + 5] == [0]
    cells = [None, b"", b"a", b"abcdefg", b"abcdefgh", b"abcdefgi", b"abcdefghi", b"abcdefghj", b"x" * 64, b"x" * 63 + b"y", b"x" * 65, b"x" * 64 + b"y"]
    got = dp(["S %d %s %d %s" % (a is None, hx(a or b""), b is None, hx(b or b"")) for a in cells for b in cells])
    assert got == [[int(R.datum_equal(a, b))] for a in cells for b in cells]


# ---------------------------------------------------------------- (4) header and binding
def test_new_symbols_resolve_and_the_abi_version_stays():
    lib = _lib.load()
    for name in ("tsq_dupcheck_create", "tsq_dupcheck_push", "tsq_dupcheck_match", "tsq_dupcheck_resolve", "tsq_dupcheck_reset", "tsq_dupcheck_stats", "tsq_dupcheck_cancel",
                 "tsq_dupcheck_destroy", "tsq_rows_equal", "tsq_chunk_append", "tsq_bytes_or"):
        assert name in abi.SIGNATURES and hasattr(lib, name), name
    assert lib.tsq_abi_version() == abi.TSQ_ABI_VERSION == 10
    assert abi.ERR_KEY_EXISTS == 16 and abi.STATUS_NAMES[16] == "KEY_EXISTS"
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    assert "TSQ_ERR_KEY_EXISTS = 16" in hdr and "#define TSQ_DUP_MAX_STREAMS 8" in hdr and "#define TSQ_ABI_VERSION 10" in hdr


def test_struct_sizes_equal_what_gcc_computes_for_the_header(tmp_path):
    import ctypes as C
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", sizeof(tsq_dup_stream), sizeof(tsq_dup_keys), '
                   'sizeof(tsq_dup_conflict), sizeof(tsq_dup_result));return 0;}\n' % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(t) for t in (abi.DupStream, abi.DupKeys, abi.DupConflict, abi.DupResult)]
