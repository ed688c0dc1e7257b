"""CPU: the sequential model of a transaction's merged read (tests/unionstore_ref.py) on the reference's own vectors
(tests/golden/unionstore_cases.json); the host build of tsq_unionstore_dp.h (sanitized, a stand-alone program) against the model —
the slot of every snapshot and buffer position, the keep rule, the limit, the lock decision, the point reads — over the edge grid, the
hand-built store of the lock outcomes and a fuzz; and the new part of the C-ABI."""
import ctypes as C
import os
import re
import subprocess

import numpy as np
import pytest

from tests import membuf_ref as MB
from tests import mvcc_ref as R
from tests import unionstore_cases as K
from tests import unionstore_ref as U
from tinysql_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
HEX = lambda b: b.hex() if b else "-"


# ------------------------------------------------------------------------------------------------ the model on the reference's vectors
@pytest.mark.parametrize("case", K.golden(), ids=[c["name"] for c in K.golden()])
def test_model_reproduces_the_references_vectors(case):
    store = K.store_of([(k.encode(), v.encode()) for k, v in case["committed"]])
    model, reads = MB.Model(), 0
    for st in case["steps"]:
        if "set" in st:
            model.Set(st["set"][0].encode(), st["set"][1].encode())
        elif "set_nil" in st:
            with pytest.raises(MB.ErrCannotSetNilValue):
                model.Set(st["set_nil"].encode(), b"")
        elif "delete" in st:
            model.Delete(st["delete"].encode())
        elif "reset" in st:
            model = MB.Model()
        elif "size" in st:
            assert (model.Size(), model.Len()) == (st["size"], st["len"])
        elif "get" in st:
            want = st["want"].encode() if st["want"] is not None else None
            assert U.get(store, model, [st["get"].encode()], K.READ_TS) == [want]
            reads += 1
        elif "iter" in st:
            got = list(U.Iter(store, model, st["iter"][0].encode(), st["iter"][1].encode(), K.READ_TS))
            assert got == [(k.encode(), v.encode()) for k, v in st["want"]]
            assert U.read(store, model, [tuple(b.encode() for b in st["iter"])], K.READ_TS)["pairs"] == got
            reads += 1
        else:
            got = list(U.IterReverse(store, model, st["iter_reverse"].encode(), K.READ_TS))
            assert got == [(k.encode(), v.encode()) for k, v in st["want"]]
            reads += 1
    assert reads


def test_the_golden_file_holds_the_vectors_of_both_test_files():
    assert [c["name"] for c in K.golden()] == ["union_store.TestGetSet", "union_store.TestDelete", "union_store.TestSeek", "union_store.TestIterReverse",
                                               "union_store.TestBasic", "buffer_store.TestGetSet", "buffer_store.TestSaveTo", "buffer_store.TestBufferStore"]


def test_model_lock_rule_by_hand():
    """the three outcomes on the hand-built store, stated without the model's help"""
    store, pushes = K.lock_store()
    d = U.Dirty(MB.replay(pushes))
    rd = lambda lo, hi, desc=False, limit=-1: K.answer(store, d, [(lo, hi)], K.READ_TS, desc, limit)
    # k10 is locked and the buffer PUTs it: the snapshot iterator steps onto it all the same, after k09 was yielded
    assert rd(b"k08", b"k12") == ("locked", b"k10", 2)
    assert rd(b"k08", b"k12", limit=2)[0] == "ok" and rd(b"k08", b"k12", limit=3)[0] == "locked"  # the limit stops it one element earlier
    assert rd(b"k10", b"k12") == ("locked", b"k10", 0) and rd(b"k10", b"k12", limit=0)[0] == "ok"
    # k39 is shadowed by a PUT: the iterator leaves it as soon as both sides meet — before the buffer's k39 is taken
    assert rd(b"k38", b"k42") == ("locked", b"k40", 1)
    assert rd(b"k38", b"k42", limit=1)[0] == "ok" and rd(b"k38", b"k42", limit=2)[0] == "locked"
    # k49 is deleted by the buffer: the same, and nothing is yielded for it
    assert rd(b"k48", b"k52") == ("locked", b"k50", 1) and rd(b"k48", b"k52", limit=1)[0] == "ok"
    # descending: k30 is met from above when k31 is left
    assert rd(b"k29", b"k33", True) == ("locked", b"k30", 2) and rd(b"k29", b"k33", True, 2)[0] == "ok"
    # Get: a buffer DEL answers without reading the snapshot; a PUT too; an untouched locked key fails
    assert K.point_answer(store, d, [b"k20", b"k10", b"k00"], K.READ_TS) == ("ok", [None, MB.replay(pushes).Get(b"k10"), K.val(b"k00")])
    assert K.point_answer(store, d, [b"k00", b"k30", b"k20"], K.READ_TS) == ("locked", b"k30", 1)


# ------------------------------------------------------------------------------------------------ the host build of tsq_unionstore_dp.h
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("unionstore_dp") / "unionstore_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "unionstore_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        return res.stdout.split("\n")
    return run


class Inputs:
    """one store and one buffer as the program reads them, and what its answers index into"""

    def __init__(self, store, pushes):
        self.store, self.dirty = store.freeze(), U.Dirty(K.model_of(pushes))
        keys, lock_keys = store.keys(), sorted(store.locks)
        self.lock_keys = lock_keys
        self.lines = ["B %d" % len(self.dirty.entries)] + ["%d %s" % (op, HEX(k)) for op, k, _ in self.dirty.entries]
        vers = [(k, v) for k in keys for v in store.versions.get(k, [])]
        self.store_pairs = [(k, v.value) for k, v in vers]
        self.lines += ["M %d %d %d" % (len(keys), len(vers), len(lock_keys))]
        self.lines += ["%s %d %d" % (HEX(k), len(store.versions.get(k, [])), lock_keys.index(k) if k in store.locks else -1) for k in keys]
        self.lines += ["%d %d" % (v.commit_ts, v.type) for _, v in vers]
        self.lines += ["%d %d %s" % (store.locks[k].start_ts, store.locks[k].op, HEX(store.locks[k].primary)) for k in lock_keys]

    def pair_of(self, tok):
        if tok[0] == "s":
            return self.store_pairs[int(tok[1:])]
        op, k, v = self.dirty.entries[int(tok[1:])]
        assert op == MB.OP_PUT
        return (k, v)


def run_reads(dp, inp, scans, gets=()):
    """scans: [(ranges, ts, desc, limit)], gets: [(keys, ts)] -> the model's answers, after the program's were held to them"""
    lines = list(inp.lines)
    for ranges, ts, desc, limit in scans:
        lines += ["Q %d %d %d %d" % (ts, 1 if desc else 0, limit, len(ranges))] + ["%s %s" % (HEX(a), HEX(b)) for a, b in ranges]
    for keys, ts in gets:
        lines += ["G %d %d" % (ts, len(keys))] + [HEX(k) for k in keys]
    out = dp(lines)
    wants = []
    for i, (ranges, ts, desc, limit) in enumerate(scans):
        head, srcs, counts = out[3 * i].split(), out[3 * i + 1].split(), out[3 * i + 2].split()
        want = K.answer(inp.store, inp.dirty, ranges, ts, desc, limit)
        wants.append(want)
        ctx = (ranges[:3], ts, desc, limit, head, want[0], want[2] if want[0] == "locked" else len(want[1]))
        assert head[0] == "R"
        if want[0] == "locked":
            assert head[1] == "17" and inp.lock_keys[int(head[3])] == want[1] and int(head[2]) == want[2], ctx
            continue
        assert head[1] == "0" and int(head[2]) == len(want[1]), ctx
        assert [inp.pair_of(t) for t in srcs] == want[1], ctx
        assert [1 if t[0] == "b" else 0 for t in srcs] == want[2], ctx
        assert [int(x) for x in counts] == want[3], ctx
        if limit != 0:
            st = U.scan_stats(inp.store, inp.dirty, ranges, ts)
            assert [int(x) for x in head[4:]] == [st[k] for k in ("positions_snapshot", "positions_buffer", "shadowed", "skipped_dels", "dangling_dels")], ctx
    at = 3 * len(scans)
    for i, (keys, ts) in enumerate(gets):
        head, verdicts = out[at + 3 * i].split(), out[at + 3 * i + 1].split()
        want = K.point_answer(inp.store, inp.dirty, keys, ts)
        wants.append(want)
        if want[0] == "locked":
            assert head[1] == "17" and inp.lock_keys[int(head[3])] == want[1] and int(head[2]) == want[2], (keys[:4], head, want)
            continue
        assert head[1] == "0" and int(head[2]) == sum(v is not None for v in want[1])
        assert [None if t in "-d" else inp.pair_of(t)[1] for t in verdicts] == want[1]
        held = dict(inp.dirty.pairs)
        assert [t == "d" for t in verdicts] == [k in held and not held[k] for k in keys]
    return wants


def total_pairs(inp, ranges, ts, desc):
    """the pairs of the read without a limit and without locks in the way (read below every lock's start_ts when one is met)"""
    want = K.answer(inp.store, inp.dirty, ranges, ts, desc, -1)
    return len(want[1]) if want[0] == "ok" else want[2]


@pytest.mark.parametrize("name,store,pushes,ranges,points", K.edge_cases(), ids=[c[0] for c in K.edge_cases()])
def test_dp_edge_grid_equals_the_model(dp, name, store, pushes, ranges, points):
    inp = Inputs(store, pushes)
    scans = []
    for desc in (False, True):
        n = total_pairs(inp, ranges, K.READ_TS, desc)
        scans += [(ranges, K.READ_TS, desc, l) for l in K.LIMITS(n) if l >= -1]
        scans += [([r], K.READ_TS, desc, -1) for r in ranges[:8]]
    scans += [([], K.READ_TS, False, -1), ([], K.READ_TS, True, 3)]
    run_reads(dp, inp, scans, [(points, K.READ_TS), ([], K.READ_TS), (points[:1], K.READ_TS)])


@pytest.mark.parametrize("name,store,pushes", K.size_grid(), ids=[c[0] for c in K.size_grid()])
def test_dp_size_grid_equals_the_model(dp, name, store, pushes):
    inp = Inputs(store, pushes)
    scans = []
    for desc in (False, True):
        n = total_pairs(inp, [(b"", b"")], K.READ_TS, desc)
        scans += [([(b"", b"")], K.READ_TS, desc, l) for l in K.LIMITS(n) if l >= -1]
    run_reads(dp, inp, scans)


def test_dp_lock_outcomes_on_the_hand_built_store(dp):
    store, pushes = K.lock_store()
    inp = Inputs(store, pushes)
    wants = run_reads(dp, inp, [(r, K.READ_TS, d, l) for r, d, l in K.lock_reads()], [(p, K.READ_TS) for p in K.lock_points()])
    assert {w[0] for w in wants} == {"ok", "locked"}
    assert {w[1] for w in wants if w[0] == "locked"} == {b"k10", b"k20", b"k30", b"k40", b"k50"}


def test_dp_fuzz_1e5_entries_1e5_keys_1000_ranges_1000_points_with_locks(dp):
    rng = np.random.default_rng(67)
    store = K.fuzz_store(rng, 100000, 400)
    pushes = K.fuzz_pushes(rng, store, 100000)
    inp = Inputs(store, pushes)
    held = dict(inp.dirty.pairs)
    assert len(store.keys()) > 50000 and len(inp.dirty.entries) > 50000 and len(set(store.keys()) & set(held)) > 10000
    ranges = K.fuzz_ranges(rng, store, inp.dirty, 1000)
    points, lock_keys = K.fuzz_points(rng, store, inp.dirty, 1000)
    LOW, HIGH = 120, 200  # below and above the locks' start_ts
    scans = []
    for desc in (False, True):
        n = total_pairs(inp, ranges, LOW, desc)
        assert n > 20000
        scans += [(ranges, ts, desc, l) for ts in (LOW, HIGH) for l in K.LIMITS(n)]
    # the lock rule: one range around every locked key, without a limit, at the count the error reports (the limit stops the iterator
    # one element earlier) and one above it
    ks = store.keys()
    at = {k: i for i, k in enumerate(ks)}
    probes = []
    for lk in lock_keys:
        i = at[lk]
        for desc in (False, True):
            r = (ks[max(0, i - 6)], ks[min(len(ks) - 1, i + 6)])
            w = K.answer(store, inp.dirty, [r], HIGH, desc, -1)
            if w[0] == "locked":
                probes += [([r], HIGH, desc, -1), ([r], HIGH, desc, w[2]), ([r], HIGH, desc, w[2] + 1)]
    del_locked = [k for k in lock_keys if k in held and not held[k]]
    gets = [(points, LOW), (points, HIGH), (points[:300] + del_locked, HIGH)] + [([ks[0], k, ks[1]], HIGH) for k in del_locked[:40]] + [([k], HIGH) for k in lock_keys[:40]]
    wants = run_reads(dp, inp, scans + probes, gets)
    # (c) the three outcomes, counted on the model's answers
    met_shadowed = sum(w[0] == "locked" and w[1] in held for w in wants[:len(scans) + len(probes)])
    stopped = 0
    for j in range(len(scans), len(scans) + len(probes), 3):
        full, at_count, above = wants[j:j + 3]
        stopped += full[0] == "locked" and full[2] > 0 and at_count[0] == "ok" and len(at_count[1]) == full[2] and above[0] == "locked"
    del_hits = sum(w[0] == "ok" for w, (keys, ts) in zip(wants[len(scans) + len(probes):], gets) if ts == HIGH and len(keys) == 3 and keys[1] in del_locked)
    assert met_shadowed >= 20 and stopped >= 20 and del_hits >= 20, (met_shadowed, stopped, del_hits)
    assert {w[0] for w in wants} == {"ok", "locked"}


# ------------------------------------------------------------------------------------------------ the new part of the C-ABI
NAMES = ("tsq_unionstore_create", "tsq_unionstore_scan", "tsq_unionstore_get", "tsq_unionstore_fetch", "tsq_unionstore_locked", "tsq_unionstore_stats",
         "tsq_unionstore_cancel", "tsq_unionstore_destroy")


def test_header_declares_the_unionstore_calls():
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    for name in NAMES:
        assert re.search(r"\b%s\(" % name, hdr) and name in abi.SIGNATURES
    assert abi.SIGNATURES["tsq_unionstore_scan"][1][-2:] == [C.POINTER(abi.UnionStoreResult), C.c_void_p]
    assert re.search(r"#define TSQ_ABI_VERSION 10\b", hdr) and abi.TSQ_ABI_VERSION == 10
    assert "tsq_mvcc_scan's convention" in hdr and "tsq_membuf_scan's" in hdr  # the header names both desc conventions side by side


def test_unionstore_struct_size_and_field_order_equal_what_gcc_computes(tmp_path):
    fields = [f for f, _ in abi.UnionStoreResult._fields_]
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu", sizeof(tsq_unionstore_result));%s return 0;}\n'
                   % (os.path.join(ROOT, "include", "tsq.h"), "".join('printf(" %%zu", offsetof(tsq_unionstore_result, %s));' % f for f in fields)))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.UnionStoreResult)] + [getattr(abi.UnionStoreResult, f).offset for f in fields]
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    assert fields == re.findall(r"\s(\w+);", re.search(r"typedef struct tsq_unionstore_result \{(.*?)\}", hdr, re.S).group(1))
    assert fields == ["n_pairs", "key_bytes", "value_bytes", "positions_snapshot", "positions_buffer", "shadowed", "skipped_dels", "dangling_dels", "from_buffer"]
