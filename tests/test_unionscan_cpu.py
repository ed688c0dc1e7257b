"""CPU: the union scan without a GPU.  (1) tests/unionscan_ref.py — the restatement every GPU test compares with — against the
reference's own rows (executor/union_scan_test.go:26-48, :75-79, :94-98).  (2) The scalar core of the kernels
(tinysql_amd/csrc/tsq_unionscan_dp.h: set build and probe, streaming bound, diagonal search, per-lane merge), built on the host as a
stand-alone sanitized program, over the tile-edge grid and the key / handle cases of the GPU tests: an index that leaves its run
stops the program.  (3) Header, binding and struct size of the new entry points."""
import ctypes as C
import os
import struct
import subprocess

import pytest

from tests import unionscan_cases as UC
from tests.unionscan_ref import UnionScanRef, canon
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


# ---------------------------------------------------------------- (1) the reference's rows
def query(snapshot, steps, used_index, desc):
    cs = UC.txn_case(snapshot, steps, used_index, desc)
    return cs.ref.run([cs.snapshot])


SNAP, GOLDEN = UC.SNAP, UC.GOLDEN


@pytest.mark.parametrize("i", range(len(GOLDEN)))
def test_restatement_gives_the_rows_of_TestDirtyTransaction(i):
    steps, used, desc, want = GOLDEN[i]
    assert query(SNAP, steps, used, desc) == want


def test_restatement_delete_all_then_insert():  # union_scan_test.go:75-79 (the handle is the hidden row id)
    snap = [(1, 1), (2, 2)]
    assert query(snap, [("delete", [1, 2])], [], False) == []
    steps = [("delete", [1, 2]), ("insert", [(3, 1)])]
    assert query(snap, steps, [], False) == [(3, 1)]
    assert query(snap, steps, [1], False) == [(3, 1)]


def test_restatement_unsigned_pk_rows():  # union_scan_test.go:92-98: a int unsigned key, rows after the readers' conditions
    types = [abi.U64, abi.I64, abi.BYTES]
    # b > 0 through idx(b, a, c): the added set holds handle 0 too, whose row the condition filtered out
    ref = UnionScanRef(types, [0, 1], [], [(1, 1, None)], [1, 0, 2], 0, False)
    assert ref.run([[]]) == [(1, 1, None)]
    # a >= 1 order by a desc, table reader
    assert UnionScanRef(types, [0, 1], [], [(1, 1, None)], [], 0, True).run([[]]) == [(1, 1, None)]
    # after insert (2, 2, null), (3, 3, 'a'): b > 1 and c is not null
    assert UnionScanRef(types, [0, 1, 2, 3], [], [(3, 3, b"a")], [1, 0, 2], 0, False).run([[]]) == [(3, 3, b"a")]


def test_DirtyTable_mirror_moves_a_deleted_handle_out_of_added():
    from tinysql_amd.executor import DirtyTable
    dt = DirtyTable()
    for h in (1, 3, 7):
        dt.AddRow(h)
    dt.DeleteRow(3)
    dt.DeleteRow(2)
    assert dt.addedRows == {1, 7} and dt.deletedRows == {2, 3}
    dt.AddRow(3)
    assert dt.addedRows == {1, 3, 7} and dt.deletedRows == {2, 3}


# ---------------------------------------------------------------- (2) the kernels' scalar core, sanitized
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("unionscan") / "unionscan_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "unionscan_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(cases, lane=8, finish=1, lanes_per_tile=256):
        """cases -> [(kept physical rows, m, take entries)]"""
        lines = []
        for cs in cases:
            lines.append("case %d %s %d %d %d %s %d %d %d" % (len(cs.types), " ".join(map(str, cs.types)), cs.handle_idx, int(cs.desc), len(cs.used_index),
                                                         " ".join(map(str, cs.used_index)), lane, lanes_per_tile, finish))
            hs = cs.added_handles + cs.deleted_handles
            lines.append("set %d %s" % (len(hs), " ".join(map(str, hs))))
            for tag, rows in (("S", cs.snapshot), ("A", cs.added_rows)):
                lines.append("%s %d" % (tag, len(rows)))
                lines += [" ".join(cell_text(tp, v) for tp, v in zip(cs.types, r)) for r in rows]
            lines.append("go")
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-300:] + res.stderr[-3000:]
        out = res.stdout.splitlines()
        assert len(out) == 2 * len(cases)
        got = []
        for i in range(len(cases)):
            kept = [int(x) for x in out[2 * i].split()[1:]]
            t = out[2 * i + 1].split()
            got.append((kept, int(t[1]), t[2:]))
        return got
    return run


def cell_text(tp, v):
    if v is None:
        return "N"
    if tp == abi.BYTES:
        return "x" + bytes(v).hex()
    if tp == abi.F64:
        return str(struct.unpack("<Q", struct.pack("<d", v))[0])
    if tp == abi.F32:
        return str(struct.unpack("<I", struct.pack("<f", v))[0])
    return str(int(v) & ((1 << 64) - 1))


def check(cs, got, finish=1):
    kept, m, take = got
    want_kept = [i for i, r in enumerate(cs.snapshot) if r in cs.ref.keep([r])]
    assert kept == want_kept, cs.name
    rows = []
    for e in take:
        assert e != "?", "%s: an output position was never written" % cs.name
        rows.append((cs.added_rows if e[0] == "a" else cs.snapshot)[int(e[1:])])
    want = cs.want()
    if not finish:
        n_det = cs.ref.determined([cs.snapshot[i] for i in want_kept])
        assert m == n_det - len(want_kept), cs.name
        want = want[:n_det]
    else:
        assert m == len(cs.added_rows)
    assert canon(cs.types, rows) == canon(cs.types, want), cs.name


@pytest.mark.parametrize("kind", UC.INTERLEAVINGS)
def test_tile_edge_grid_on_the_host(dp, kind):
    cases = [UC.table_case(kind, t) for t in UC.TILE_TOTALS] + [UC.table_case(kind, t, desc=True) for t in (65, 4097)]
    for cs, got in zip(cases, dp(cases)):
        check(cs, got)


@pytest.mark.parametrize("lane,lanes_per_tile", [(1, 1), (1, 256), (3, 5), (8, 1), (8, 16), (4096, 2)])
def test_lane_and_tile_widths_and_the_streaming_bound_on_the_host(dp, lane, lanes_per_tile):
    cases = [UC.table_case(k, t) for k in ("alternate", "added_last", "runs_1000", "one_added_mid") for t in (2, 257, 4097)]
    for finish in (0, 1):
        for cs, got in zip(cases, dp(cases, lane=lane, finish=finish, lanes_per_tile=lanes_per_tile)):
            check(cs, got, finish)


def key_cases():
    out = []
    for desc in (False, True):
        out += [UC.one_key_case(tp, desc) for tp in (abi.I64, abi.U64, abi.F32, abi.F64, abi.BYTES)]
        out += [UC.multi_key_case(2, desc), UC.multi_key_case(4, desc), UC.payload_case(desc)]
        out += [UC.edge_handle_case(tp, desc, w) for tp in (abi.I64, abi.U64) for w in (0, 1)]
    return out + [UC.colliding_case()]


def test_keys_handles_and_collisions_on_the_host(dp):
    cases = key_cases()
    for finish in (0, 1):
        for cs, got in zip(cases, dp(cases, finish=finish)):
            check(cs, got, finish)


def test_unsorted_input_keeps_every_index_in_range(dp):
    # the contract is sorted input; for anything else the rows are unspecified but the sanitizers must stay silent
    import random
    rng = random.Random(3)
    cases = []
    for t in (2, 65, 1025, 4097):
        cs = UC.table_case("alternate", t)
        rng.shuffle(cs.snapshot)
        rng.shuffle(cs.added_rows)
        cases.append(cs)
    for lane, lpt in ((1, 4), (8, 256), (8, 3)):
        for finish in (0, 1):
            for cs, (kept, m, take) in zip(cases, dp(cases, lane=lane, finish=finish, lanes_per_tile=lpt)):
                assert 0 <= m <= len(cs.added_rows) and len(take) == len(kept) + m


# ---------------------------------------------------------------- (3) the C-ABI
def test_new_abi_is_declared_exported_and_the_version_stays():
    assert abi.TSQ_ABI_VERSION == 10
    lib = _lib.load()
    names = ["tsq_unionscan_" + n for n in ("set_slots", "create", "set_added", "push", "finish", "peek", "pull", "stats", "cancel", "destroy")]
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    for name in names:
        assert name in abi.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert lib.tsq_abi_version() == 10
    for n in (0, 1, 31, 32, 33, 1000, 1 << 20):
        assert lib.tsq_unionscan_set_slots(n) == UC.set_slots(n)


def test_cfg_size_equals_what_gcc_computes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu\\n", sizeof(tsq_unionscan_cfg));return 0;}\n' % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    assert int(subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout) == C.sizeof(abi.UnionScanCfg)
