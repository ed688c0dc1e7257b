"""CPU: the index lookup without a GPU.  (1) tests/lookup_ref.py — the restatement every GPU test compares with — against the
reference's own double-read rows (tests/golden/index_lookup_cases.json).  (2) The scalar core of the search kernel
(tinysql_amd/csrc/tsq_lookup_dp.h: index plan, sampling, descent), built on the host as a stand-alone sanitized program and compared
with np.searchsorted over the stride x table-size grid: an index that leaves its level stops the program.  (3) Header and binding of
the new entry points."""
import os
import re
import subprocess

import numpy as np
import pytest

from tests import lookup_ref as LR
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
CASES = LR.load_cases()


# ---------------------------------------------------------------- (1) the reference's rows
@pytest.mark.parametrize("case", CASES, ids=[c["name"] for c in CASES])
def test_restatement_gives_the_rows_of_the_reference(case):
    assert re.match(r"executor/\w+_test\.go:\d+", case["source"])
    rows = LR.run_case(case)
    assert rows == case["reader_rows"]
    assert LR.apply_parent(case, rows) == case["query_rows"]
    if case["keep_order"]:  # the output does not depend on how the handles were cut into tasks
        for init, mx in ((1, 3), (3, 3), (1, 1 << 20), (2, 2)):
            assert LR.run_case(case, init, mx) == case["reader_rows"]


def test_task_cut_doubles_after_full_tasks_up_to_the_maximum():
    sizes = lambda n, i, m: [b - a for a, b in LR.cut_tasks(n, i, m)]  # noqa: E731
    assert sizes(10, 1024, 3) == [3, 3, 3, 1]  # executor_test.go:559-566
    assert sizes(100, 1, 16) == [1, 2, 4, 8, 16, 16, 16, 16, 16, 5]
    assert sizes(7, 4, 1 << 20) == [4, 3]
    assert sizes(12, 4, 1 << 20) == [4, 8]
    assert sizes(0, 4, 8) == []
    assert [c["tasks"] for c in CASES if "tasks" in c] == [[3, 3, 3, 1]]


def test_restatement_duplicates_missing_and_extremes():
    table = np.array([I64_MIN, -5, 0, 7, I64_MAX], dtype=np.int64)
    task = np.array([7, I64_MAX, 3, 7, I64_MIN, -6], dtype=np.int64)
    rows, hs = LR.lookup_task(table, task, False)
    assert rows.tolist() == [0, 3, 3, 4] and hs.tolist() == [I64_MIN, 7, 7, I64_MAX]
    rows, hs = LR.lookup_task(table, task, True)  # the pinned departure: each occurrence at its own position
    assert rows.tolist() == [3, 4, 3, 0] and hs.tolist() == [7, I64_MAX, 7, I64_MIN]
    assert LR.as_i64([(1 << 63) + 5]).tolist() == [I64_MIN + 5]  # an unsigned PK beyond 2^63 - 1: its raw bytes, signed order


# ---------------------------------------------------------------- (2) the kernel's scalar core, sanitized
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("lookup") / "lookup_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "lookup_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(table, queries, runs):
        """runs: [(op, shift, top_max)] -> [(levels, positions)]"""
        lines = ["T %d %s" % (len(table), " ".join(map(str, table.tolist()))), "Q %d %s" % (len(queries), " ".join(map(str, queries.tolist())))]
        lines += ["%s %d %d" % r for r in runs]
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        out = [ln.split() for ln in res.stdout.splitlines()]
        assert len(out) == len(runs)
        return [(int(t[0]), np.array(t[1:], dtype=np.int64)) for t in out]
    return run


def make_table(n, seed):
    """n strictly ascending handles with both int64 extremes and runs of consecutive values"""
    if n == 0:
        return np.zeros(0, np.int64)
    rng = np.random.default_rng(seed)
    gaps = rng.integers(1, 1 << 40, n).astype(np.int64)
    gaps[rng.random(n) < 0.5] = 1  # runs of consecutive handles
    t = -(1 << 50) + np.cumsum(gaps)
    if n >= 1:
        t[-1] = I64_MAX
    if n >= 2:
        t[0] = I64_MIN
    return t.astype(np.int64)


def make_queries(t):
    """every handle, every handle +- 1 without wrapping, both extremes"""
    below = t[t > I64_MIN] - 1
    above = t[t < I64_MAX] + 1
    return np.concatenate([t, below, above, np.array([I64_MIN, I64_MAX], dtype=np.int64)])


def table_sizes(s):
    S = 1 << s
    return sorted({0, 1, 2, S - 1, S, S + 1, S * S - 1, S * S + 1, 70001} - {-1})


@pytest.mark.parametrize("shift", [1, 2, 3, 4, 5, 6])
def test_sampled_search_equals_searchsorted_on_the_host(dp, shift):
    for n in table_sizes(shift):
        t = make_table(n, 100 * shift + n % 97)
        assert n < 2 or (np.diff(t.astype(object)) > 0).all()
        q = make_queries(t)
        want = np.searchsorted(t, q, side="left")
        # the library's top level (1024 entries), a tiny one (every level of the descent in use), and no index at all
        runs = [("S", shift, 1024), ("S", shift, 1), ("S", 0, 1024), ("F", shift, 4)]
        got = dp(t, q, runs)
        for (op, s, top), (levels, pos) in zip(runs, got):
            if op == "S":
                assert (pos == want).all(), (n, s, top)
            else:
                hit = want < n
                hit[hit] = t[want[hit]] == q[hit]
                assert (pos == np.where(hit, want, -1)).all(), (n, s, top)
        assert got[2][0] == 0
        if n > 1024:
            assert got[0][0] >= 1
        if n > 4 << shift:
            assert got[1][0] >= 2  # several levels on small tables


def test_plan_never_exceeds_its_level_limit(dp):
    t = make_table(70001, 5)
    q = make_queries(t)[::7]
    (levels, pos), = dp(t, q, [("S", 1, 1)])  # 2-entry strides stop at 8 levels: the top level is then searched as it is
    assert levels == 8 and (pos == np.searchsorted(t, q, side="left")).all()


# ---------------------------------------------------------------- (3) the C-ABI
NAMES = ["tsq_lookup_create", "tsq_lookup_task", "tsq_lookup_stats", "tsq_lookup_cancel", "tsq_lookup_destroy", "tsq_rows_gather"]


def test_new_abi_is_declared_exported_and_the_version_stays():
    assert abi.TSQ_ABI_VERSION == 10
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    for name in NAMES:
        assert name in abi.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert lib.tsq_abi_version() == 10
    assert re.search(r"#define TSQ_KNOB_LOOKUP_STRIDE 46\b", hdr) and re.search(r"#define TSQ_KNOB_GATHER_WAVE_COPY 47\b", hdr)
    assert re.search(r"TSQ_KNOB_COUNT = 48\b", hdr)
    assert (abi.KNOB_LOOKUP_STRIDE, abi.KNOB_GATHER_WAVE_COPY) == (46, 47)


def test_ctypes_prototypes_match_the_header():
    """argument count and the kind of every argument (pointer / 32-bit / 64-bit / double) of the new entry points"""
    import ctypes as C
    hdr = re.sub(r"/\*.*?\*/", "", open(os.path.join(ROOT, "include", "tsq.h")).read(), flags=re.S)
    for name in NAMES:
        m = re.search(r"(\w+)\s+" + name + r"\(([^;]*)\);", hdr)
        assert m, name
        restype, argtypes = abi.SIGNATURES[name]
        assert (restype is None) == (m.group(1) == "void")
        args = [a.strip() for a in m.group(2).split(",")]
        assert len(args) == len(argtypes), name
        for a, ct in zip(args, argtypes):
            if "*" in a:
                assert ct is C.c_void_p or hasattr(ct, "contents") or issubclass(ct, C._Pointer), (name, a)
            elif a.startswith("int64_t"):
                assert ct is C.c_int64, (name, a)
            elif a.startswith("int32_t"):
                assert ct is C.c_int32, (name, a)
            elif a.startswith("uint32_t"):
                assert ct is C.c_uint32, (name, a)
            else:
                raise AssertionError("unexpected argument %r of %s" % (a, name))
