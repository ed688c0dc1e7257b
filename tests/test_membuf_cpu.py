"""CPU: the dict model of the transaction buffer (tests/membuf_ref.py) against the reference's own tests
(tests/golden/membuf_cases.json), the host build of tsq_membuf_dp.h (sanitized, a stand-alone program) against the model — the push
checks, the order in the lane and the wave form, the winner rule, the search of a Get — and the new part of the C-ABI."""
import bisect
import ctypes as C
import json
import os
import re
import subprocess

import numpy as np
import pytest

from tests import membuf_cases as MC
from tests import membuf_ref as MR
from tinysql_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
L1 = lambda s: s.encode("latin-1")
HEX = lambda b: b.hex() if b else "-"


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "membuf_cases.json")))


def seek(m, k):
    """memDbBuffer.Iter(k, nil).Key(): the smallest key at or above k, None when the iterator is invalid"""
    keys = [kv[0] for kv in m.walk()]
    i = bisect.bisect_left(keys, k)
    return keys[i] if i < len(keys) else None


# ------------------------------------------------------------------------------------------------ the model on the reference's vectors
def test_model_get_set():
    g = golden()["get_set"]
    m = MR.Model()
    for k, v in g["sets"]:
        m.Set(L1(k), L1(v))
    for k, v in g["gets"]:
        assert m.Get(L1(k)) == L1(v)
    with pytest.raises(MR.ErrNotExist):
        m.Get(b"0000000001")


def test_model_new_iterator():
    g = golden()["new_iterator"]
    m = MR.Model()
    assert seek(m, b"") is None  # "should be invalid"
    for k, v in g["sets"]:
        m.Set(L1(k), L1(v))
    assert [k for k, _ in m.walk()] == [L1(k) for k in g["walk"]]
    for k, want in g["seeks"]:
        assert seek(m, L1(k)) == (None if want is None else L1(want))


def test_model_new_iterator_min():
    g = golden()["new_iterator_min"]
    m = MR.Model()
    for k, v in reversed(g["sets"]):  # (any push order: the walk is sorted)
        m.Set(L1(k), L1(v))
    assert m.Len() == g["count"] == len(m.walk())
    assert [k for k, _ in m.walk()] == [L1(k) for k, _ in g["sets"]]
    ks = [L1(k) for k, _ in g["sets"]]
    assert sum(1 for a in ks for b in ks if a != b and b.startswith(a)) == 4  # keys 0 and 3 are proper prefixes of two others each
    for k, want in g["seeks"]:
        assert seek(m, L1(k)) == L1(want)


def test_model_buffer_limit_is_sequential():
    g = golden()["buffer_limit"]
    m = MR.Model(g["entry_size_limit"], g["total_size_limit"])
    for k, vlen, want in g["sets"]:
        if want is None:
            m.Set(L1(k), bytes(vlen))
        else:
            with pytest.raises((MR.ErrEntryTooLarge, MR.ErrTxnTooLarge)):
                m.Set(L1(k), bytes(vlen))
    assert m.Len() == 1 and m.Size() == 500
    # the buffer limit proper, which the third Set of the reference's test never reaches: the Set is IN when the error comes
    m = MR.Model(0, 1000)
    m.Set(b"x", bytes(499))
    with pytest.raises(MR.ErrTxnTooLarge):
        m.Set(b"y", bytes(500))
    assert m.Len() == 2 and m.Size() == 1001
    with pytest.raises(MR.ErrTxnTooLarge):  # what tsq_membuf_finish answers instead: one check of the final size
        m.finish()
    with pytest.raises(MR.ErrCannotSetNilValue):
        m.Set(b"z", b"")


def test_model_mutations_ops_size_and_primary():
    m = MR.replay(dict(MC.order_cases())["orders_one_buffer"])
    got = m.finish()
    ops = {k: op for op, k, _ in got["entries"]}
    assert ops == {b"k-a": MR.OP_DEL, b"k-b": MR.OP_PUT, b"k-c": MR.OP_PUT, b"k-d": MR.OP_PUT, b"k-e": MR.OP_LOCK, b"k-f": MR.OP_LOCK}
    assert (got["puts"], got["dels"], got["locks"]) == (3, 1, 2) and got["primary"] == b"k-a" and got["primary_index"] == 0
    assert got["size"] == sum(len(k) + len(v) for _, k, v in got["entries"])
    assert [e[1] for e in got["entries"]] == sorted(ops)
    lock_only = MR.replay(dict(MC.order_cases())["lock_only"]).finish()
    assert [e[1] for e in lock_only["entries"]] == [b"p", b"q", b"r"] and lock_only["primary"] == b"q" and lock_only["primary_index"] == 1
    later = MR.replay(dict(MC.order_cases())["lock_then_smaller_put"]).finish()
    assert later["primary"] == b"m" and later["primary_index"] == 1
    assert MR.Model().finish()["primary_index"] == -1


# ------------------------------------------------------------------------------------------------ the host build of tsq_membuf_dp.h
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("membuf_dp") / "membuf_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "membuf_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        return res.stdout.split("\n")
    return run


def buffer_lines(pushes, entry_limit=0):
    out = ["B %d %d" % (entry_limit, len(pushes))]
    for kind, keys, values in pushes:
        out.append("P %d %d" % (kind, len(keys)))
        out += ["%s %d" % (HEX(k), len(values[i]) if values is not None else 0) for i, k in enumerate(keys)]
    return out


def last_writer(pushes):
    """{key: sequence number of the entry that must survive}: the last Set or Delete, else the last lock"""
    best, seq = {}, 0
    for kind, keys, _ in pushes:
        for k in keys:
            rank = (kind != MR.LOCK, seq)
            if k not in best or rank > best[k]:
                best[k] = rank
            seq += 1
    return {k: r[1] for k, r in best.items()}


def parse_result(out, at=0):
    """-> (header ints, [(op, key, value length, sequence number)], the line behind them)"""
    while not out[at].startswith("R "):
        at += 1
    head = [int(x) for x in out[at].split()[1:]]
    rows = []
    for line in out[at + 1:at + 1 + head[0]]:
        op, k, vl, seq = line.split()
        rows.append((int(op), b"" if k == "-" else bytes.fromhex(k), int(vl), int(seq)))
    return head, rows, at + 1 + head[0]


def check_against_model(dp, pushes, probes=()):
    model = MR.replay(pushes).finish()
    out = dp(buffer_lines(pushes) + ["G %d" % len(probes)] + [HEX(p) for p in probes])
    assert not any(l.startswith("E ") for l in out)
    head, rows, at = parse_result(out)
    assert [(op, k, vl) for op, k, vl, _ in rows] == [(op, k, len(v)) for op, k, v in model["entries"]]
    want_seq = last_writer(pushes)
    assert [seq for _, _, _, seq in rows] == [want_seq[k] for _, k, _ in model["entries"]]
    all_keys = [k for _, ks, _ in pushes for k in ks]
    ascending = all(a < b for a, b in zip(all_keys, all_keys[1:]))
    assert head[3] == int(ascending)
    if ascending:
        assert head[4] == 0
    if all_keys:
        assert head[1] == len(os.path.commonprefix(all_keys)) and head[2] == (max(map(len, all_keys)) - head[1] + 7) // 8
    assert out[at] == "G"
    keys = [k for _, k, _ in model["entries"]]
    assert [int(x) for x in out[at + 1:at + 1 + len(probes)]] == [keys.index(p) if p in keys else -1 for p in probes]
    return head


@pytest.mark.parametrize("name,pushes", MC.all_small_cases(), ids=[c[0] for c in MC.all_small_cases()])
def test_dp_edge_grid_equals_the_model(dp, name, pushes):
    keys = sorted({k for _, ks, _ in pushes for k in ks})
    probes = keys[::max(1, len(keys) // 40)] + [b"\x00", b"\xff" * 9] + [k + b"\x00" for k in keys[:5]] + [k[:-1] for k in keys[:5] if len(k) > 1]
    check_against_model(dp, pushes, probes)


def test_dp_fuzz_1e5_keys_three_letter_alphabet(dp):
    pushes = MC.fuzz_pushes(np.random.default_rng(47), 100000)
    assert sum(len(ks) for _, ks, _ in pushes) == 100000
    distinct = {k for _, ks, _ in pushes for k in ks}
    assert len(distinct) < 30000 and any(k.endswith(b"\x00") and k[:-1] in distinct for k in distinct)  # heavy duplicates, trailing-zero twins
    head = check_against_model(dp, pushes, sorted(distinct)[::500] + [b"c"])
    assert head[4] > 0


def test_dp_ascending_entries_need_no_pass(dp):
    ks = MC.record_keys(41, range(-300, 300))
    head = check_against_model(dp, [MC.sets(ks[:256], 0, 38), MC.sets(ks[256:], 256, 38)], ks[::50])
    assert head[1:5] == [11, 1, 1, 0]  # 11 shared bytes, one image, ascending, no pass


def test_dp_push_refusals(dp):
    out = dp(buffer_lines([(MR.SET, [b"a", b"", b"c"], [b"1", b"2", b"3"]), (MR.SET, [b"a", b"b"], [b"1", b""]), (MR.DELETE, [b"d", b""], None),
                           (MR.SET, [b"k", b"kk", b"kkk"], [bytes(9), bytes(9), bytes(7)]), (MR.SET, [b"ok"], [b"v"])], entry_limit=10))
    assert [l for l in out if l.startswith("E ")] == ["E 0 2 1", "E 1 4 1", "E 2 2 1", "E 3 8 1"]
    head, rows, _ = parse_result(out)
    assert rows == [(MR.OP_PUT, b"ok", 1, 0)]  # the refused pushes added nothing: the one entry has sequence number 0
    assert MR.first_refused_row(MR.SET, [b"k", b"kk", b"kkk"], [bytes(9), bytes(9), bytes(7)], 10) == 1


# ------------------------------------------------------------------------------------------------ the new part of the C-ABI
def test_header_declares_the_membuf_calls_and_kinds():
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    for name in ("create", "push", "finish", "request", "get", "destroy"):
        assert re.search(r"\btsq_membuf_%s\(" % name, hdr) and "tsq_membuf_%s" % name in abi.SIGNATURES
    for name, val in (("SET", abi.MEMBUF_SET), ("DELETE", abi.MEMBUF_DELETE), ("LOCK", abi.MEMBUF_LOCK)):
        assert int(re.search(r"#define TSQ_MEMBUF_%s (\d+)" % name, hdr).group(1)) == val
    assert (abi.MEMBUF_SET, abi.MEMBUF_DELETE, abi.MEMBUF_LOCK) == (MR.OP_PUT, MR.OP_DEL, MR.OP_LOCK)  # a kind is its op
    assert re.search(r"#define TSQ_ABI_VERSION 10\b", hdr) and abi.TSQ_ABI_VERSION == 10


def test_membuf_struct_sizes_equal_what_gcc_computes_for_the_header(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", sizeof(tsq_membuf_cfg), '
                   'sizeof(tsq_membuf_result), offsetof(tsq_membuf_cfg, flags), offsetof(tsq_membuf_result, kernel_ms));return 0;}\n'
                   % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.MembufCfg), C.sizeof(abi.MembufResult), abi.MembufCfg.flags.offset, abi.MembufResult.kernel_ms.offset]
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    assert [f for f, _ in abi.MembufResult._fields_] == re.findall(r"\s(\w+);", re.search(r"typedef struct tsq_membuf_result \{(.*?)\}", hdr, re.S).group(1))
