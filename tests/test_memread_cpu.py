"""CPU: the restatement of the mem readers (tests/memread_ref.py) on the reference's own rows (tests/golden/memread_cases.json), the two
models of the dirty handles, the host build of tsq_memread_dp.h (sanitized, a stand-alone program) against the restatement — range
bounds, point reads, position -> (range, entry), the keep rule, the ascending and descending placement, the dirty-handle pass — and
the new part of the C-ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import membuf_cases as MC
from tests import membuf_ref as MR
from tests import memread_cases as K
from tests import memread_ref as R
from tests.unionscan_ref import UnionScanRef
from tinysql_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEX = lambda b: b.hex() if b else "-"


# ------------------------------------------------------------------------------------------------ the model on the reference's rows
@pytest.mark.parametrize("case", K.golden(), ids=[c["name"] for c in K.golden()])
def test_model_reads_the_fixture_rows(orc, case):
    layout, model = K.Layout(case["table"]), MR.Model()
    txn = K.Txn(orc, layout, case["committed"], [model])
    reads = 0
    for step in case["steps"]:
        if "insert" in step:
            txn.insert(step["insert"])
        elif "delete" in step:
            txn.delete(step["delete"])
        else:
            rd = K.Read(layout, txn, step["read"])
            added, deleted = R.dirty_sets(model, layout.id)
            # the buffer's sets and the sequential DirtyTable's: the union is what getSnapshotRow reads, and it is the same
            assert set(added) | set(deleted) == txn.dirty.addedRows | txn.dirty.deletedRows
            rows = UnionScanRef(rd.types, added, deleted, rd.model_rows(orc, layout, model), rd.used_index, rd.handle_idx, rd.desc).run([rd.snapshot])
            assert rd.project(rows) == rd.expect, step
            reads += 1
    assert reads


def test_dirty_sets_differ_from_dirty_table_on_delete_then_insert(orc):
    """pinned departure 2: a handle deleted and then re-inserted is in BOTH of DirtyTable's sets, here in `added` only; the unions agree"""
    case = K.golden()[0]
    layout, model = K.Layout(case["table"]), MR.Model()
    txn = K.Txn(orc, layout, case["committed"], [model])
    txn.delete([2])
    txn.insert([[2, 2, 9]])
    added, deleted = R.dirty_sets(model, layout.id)
    assert (added, deleted) == ([2], [])
    assert (txn.dirty.addedRows, txn.dirty.deletedRows) == ({2}, {2})
    assert set(added) | set(deleted) == txn.dirty.addedRows | txn.dirty.deletedRows
    # insert-then-delete of a new handle: the sequential model forgets the insert, the buffer keeps the delete — both have it deleted only
    txn.insert([[9, 9, 1]])
    txn.delete([9])
    added, deleted = R.dirty_sets(model, layout.id)
    assert 9 in deleted and 9 not in added and 9 in txn.dirty.deletedRows and 9 not in txn.dirty.addedRows


def test_model_iter_skips_deletes_and_lock_only_keys():
    m = MR.replay([MC.sets([b"a", b"b", b"c", b"e"]), MC.deletes([b"b"]), MC.locks([b"d", b"a"])])
    got = R.scan(m, [(b"", b""), (b"b", b"e"), (b"c", b"c"), (b"x", b"a")])
    assert [k for k, _ in got["pairs"]] == [b"a", b"c", b"e", b"c"]
    assert got["range_counts"] == [3, 1, 0, 0] and got["positions"] == 5 + 3 and got["skipped_dels"] == 2
    assert [k for k, _ in R.scan(m, [(b"", b""), (b"b", b"e")], desc=True)["pairs"]] == [b"c", b"e", b"c", b"a"]  # the WHOLE sequence reversed
    pts = R.scan_points(m, [b"e", b"b", b"d", b"zz", b"a", b"e"])
    assert [k for k, _ in pts["pairs"]] == [b"e", b"a", b"e"] and pts["positions"] == 5 and pts["skipped_dels"] == 1


# ------------------------------------------------------------------------------------------------ the host build of tsq_memread_dp.h
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("memread_dp") / "memread_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "memread_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        return res.stdout.split("\n")
    return run


def buffer_lines(model):
    ents = R.entries(model)
    return ["B %d" % len(ents)] + ["%d %s %d" % (op, HEX(k), len(v)) for op, k, v in ents]


def parse_scan(out, at):
    """-> (the five counts, the range counts, [(entry, key offset, value offset)], the line behind them)"""
    head = [int(x) for x in out[at].split()[1:]]
    assert out[at].startswith("S ") and out[at + 1].startswith("C")
    counts = [int(x) for x in out[at + 1].split()[1:]]
    rows = [tuple(int(x) for x in l.split()) for l in out[at + 2:at + 2 + head[0]]]
    return head, counts, rows, at + 2 + head[0]


def check_scan(model, want, got):
    """the program's answer against the restatement's: the counts, and per pair the entry and where its bytes begin"""
    head, counts, rows = got
    ents = R.entries(model)
    assert head == [len(want["pairs"]), sum(len(k) for k, _ in want["pairs"]), sum(len(v) for _, v in want["pairs"]), want["positions"], want["skipped_dels"]]
    assert counts == want["range_counts"]
    assert [(ents[e][1], ents[e][2]) for e, _, _ in rows] == want["pairs"]
    ko = np.concatenate([[0], np.cumsum([len(k) for k, _ in want["pairs"]])])[:-1].tolist() if rows else []
    vo = np.concatenate([[0], np.cumsum([len(v) for _, v in want["pairs"]])])[:-1].tolist() if rows else []
    assert [r[1] for r in rows] == ko and [r[2] for r in rows] == vo


def run_scans(dp, model, range_lists, point_lists=()):
    lines = buffer_lines(model)
    for desc, ranges in range_lists:
        lines += ["S %d %d" % (desc, len(ranges))] + ["%s %s" % (HEX(a), HEX(b)) for a, b in ranges]
    for keys in point_lists:
        lines += ["P %d" % len(keys)] + [HEX(k) for k in keys]
    out = dp(lines)
    at = 0
    for desc, ranges in range_lists:
        head, counts, rows, at = parse_scan(out, at)
        check_scan(model, R.scan(model, ranges, bool(desc)), (head, counts, rows))
    for keys in point_lists:
        head, counts, rows, at = parse_scan(out, at)
        check_scan(model, R.scan_points(model, keys), (head, counts, rows))


@pytest.mark.parametrize("name,pushes", MC.all_small_cases(), ids=[c[0] for c in MC.all_small_cases()])
def test_dp_edge_grid_equals_the_model(dp, name, pushes):
    model = MR.replay(pushes)
    keys = [e[1] for e in R.entries(model)]
    if not keys:
        run_scans(dp, model, [(0, []), (0, [(b"", b"")]), (1, [(b"a", b"")])], [[], [b"a"]])
        return
    rs = K.edge_ranges(keys)
    pts = keys[::max(1, len(keys) // 30)] + [b"\x00", b"\xff" * 9, keys[0] + b"\x00", keys[-1][:-1] or b"q", keys[0], keys[0]]
    run_scans(dp, model, [(0, rs), (1, rs), (0, []), (1, rs[:1])], [pts, []])


def test_dp_fuzz_1e5_keys_three_letter_alphabet_1000_ranges(dp):
    rng = np.random.default_rng(53)
    pushes = MC.fuzz_pushes(rng, 100000)
    model = MR.replay(pushes)
    ents = R.entries(model)
    keys = [e[1] for e in ents]
    assert len(keys) > 10000 and {e[0] for e in ents} == {MR.OP_PUT, MR.OP_DEL, MR.OP_LOCK}
    ranges = []
    for _ in range(1000):  # ends drawn from the stored keys, a few ranks apart (either way round), and from strings the buffer does not hold
        i = int(rng.integers(0, len(keys)))
        j = min(len(keys) - 1, max(0, i + int(rng.integers(-20, 200))))
        a, b = keys[i], keys[j]
        if rng.random() < 0.3:
            a = a[:int(rng.integers(0, len(a) + 1))]
        if rng.random() < 0.3:
            b = b + bytes(rng.choice([0x00, 0x61, 0x62], int(rng.integers(1, 3))).astype(np.uint8))
        ranges.append((a, b))
    pts = [keys[int(i)] for i in rng.integers(0, len(keys), 500)] + [bytes(rng.choice([0x00, 0x61, 0x62], 7).astype(np.uint8)) for _ in range(500)]
    run_scans(dp, model, [(0, ranges), (1, ranges)], [pts])


def test_dp_dirty_handles(dp):
    edge = [-(1 << 63), -1, 0, 1, (1 << 63) - 1]
    tid = 41
    pushes = [MC.sets(MC.record_keys(tid, edge + [7, 8, 9]), 0, 38), MC.deletes(MC.record_keys(tid, [8, 100, -5])), MC.locks(MC.record_keys(tid, [9, 200])),
              MC.sets(MC.record_keys(tid - 1, [1, 2]) + MC.record_keys(tid + 1, [3]), 50, 38), MC.deletes(MC.record_keys(tid + 1, [4])),
              MC.sets([R.index_prefix(tid, 1) + b"\x03abc", R.index_prefix(tid, 2) + R.flip(5)], 60, 8)]
    model = MR.replay(pushes)
    want = R.dirty_sets(model, tid)
    assert want == (sorted(edge + [7, 9]), [-5, 8, 100])  # (9: the Set wins over the lock; 200: lock-only, in neither list)
    out = dp(buffer_lines(model) + ["D %d" % tid, "D %d" % (tid + 1), "D %d" % (tid + 7)])
    assert out[0] == "D %d %d" % (len(want[0]), len(want[1]))
    assert ([int(x) for x in out[1].split()], [int(x) for x in out[2].split()]) == want
    assert out[3] == "D 1 1" and out[4].split() == ["3"] and out[5].split() == ["4"]
    assert out[6] == "D 0 0"
    bad = MR.replay(pushes + [MC.sets([R.record_key(tid, 5) + b"\x00"], 70, 3)])  # a 20-byte key inside the record range
    with pytest.raises(R.InvalidKey):
        R.dirty_sets(bad, tid)
    assert dp(buffer_lines(bad) + ["D %d" % tid])[0] == "E invalid key"


# ------------------------------------------------------------------------------------------------ the new part of the C-ABI
def test_header_declares_the_memread_calls():
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    for name in ("tsq_membuf_scan", "tsq_membuf_scan_points", "tsq_membuf_fetch", "tsq_membuf_dirty", "tsq_membuf_dirty_fetch", "tsq_unionscan_create_dev"):
        assert re.search(r"\b%s\(" % name, hdr) and name in abi.SIGNATURES
    assert abi.SIGNATURES["tsq_unionscan_create_dev"][1][1:] == [C.POINTER(abi.UnionScanCfg), C.c_void_p, C.c_int64, C.c_void_p, C.c_int64, C.POINTER(C.c_void_p)]
    assert re.search(r"#define TSQ_ABI_VERSION 10\b", hdr) and abi.TSQ_ABI_VERSION == 10


def test_memread_struct_size_equals_what_gcc_computes_for_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu\\n", sizeof(tsq_membuf_scan_result), '
                   'offsetof(tsq_membuf_scan_result, skipped_dels));return 0;}\n' % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.MembufScanResult), abi.MembufScanResult.skipped_dels.offset]
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    assert [f for f, _ in abi.MembufScanResult._fields_] == re.findall(r"\s(\w+);", re.search(r"typedef struct tsq_membuf_scan_result \{(.*?)\}", hdr, re.S).group(1))
