"""CPU: the group-id dictionary (tsq_groupid_*) and tsq_agg_create_keys are declared, bound and exported without an ABI change, their
constructors refuse a NULL context, and the cell semantics of csrc/tsq_groupid_dp.h agree with the oracle's group-key encoding."""
import ctypes as C
import os
import struct
import subprocess

import numpy as np

from tests import groupid_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Column, StrColumn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
NAMES = ["tsq_groupid_create", "tsq_groupid_assign", "tsq_groupid_count", "tsq_groupid_keys", "tsq_groupid_stats", "tsq_groupid_cancel",
         "tsq_groupid_destroy", "tsq_agg_create_keys"]


def test_groupid_symbols_are_bound_and_exported():
    lib = _lib.load()
    for name in NAMES:
        assert name in abi.SIGNATURES, name
        assert hasattr(lib, name), "libtsq.so does not export %s" % name
    assert abi.GROUPID_MAX_KEYS == 16


def test_abi_version_is_still_10():
    assert abi.TSQ_ABI_VERSION == 10
    assert _lib.load().tsq_abi_version() == 10


def test_agg_cfg_size_equals_what_gcc_computes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include "%s"\nint main(){printf("%%zu %%d\\n", sizeof(tsq_agg_cfg), TSQ_GROUPID_MAX_KEYS);return 0;}\n'
                   % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.AggCfg), abi.GROUPID_MAX_KEYS]


def test_constructors_with_a_null_context_are_invalid_and_leave_out_alone():
    lib = _lib.load()
    types = (C.c_int32 * 5)(*[abi.I64] * 5)
    out = C.c_void_p(0x1234)
    assert lib.tsq_groupid_create(None, types, 5, 0, C.byref(out)) == abi.ERR_INVALID
    assert out.value == 0x1234
    cfg = abi.AggCfg()
    cfg.n_aggs, cfg.n_input_cols = 1, 5
    cfg.aggs[0].func, cfg.aggs[0].arg_col = abi.AGG_COUNT, -1
    cols = (C.c_int32 * 5)(0, 1, 2, 3, 4)
    assert lib.tsq_agg_create_keys(None, C.byref(cfg), cols, types, 5, C.byref(out)) == abi.ERR_INVALID
    assert out.value == 0x1234


def _f32(bits):
    return struct.unpack("<f", struct.pack("<I", bits))[0]


def _f64(bits):
    return struct.unpack("<d", struct.pack("<Q", bits))[0]


def cell_table():
    """(type, [cells]): every pair of cells of one type is compared.  A cell: None (NULL), an int / float, or bytes."""
    nan_a, nan_b = 0x7ff8000000000001, 0x7ff8000000000002
    return [
        (abi.I64, [None, 0, 1, -1, -(1 << 63), (1 << 63) - 1]),
        (abi.U64, [None, 0, 1, 1 << 63, (1 << 64) - 1]),  # 2^63 in a U64 column ...
        (abi.I64, [-(1 << 63), 0, None]),                 # ... and -2^63 in an I64 column: the same 8 bytes, each among its own type
        (abi.F64, [None, 0.0, -0.0, 1.5, -1.5, _f64(nan_a), _f64(nan_b), _f64(nan_a), float("inf"), -float("inf")]),
        # F32: +-0, two NaN payloads, and 16777216 = 2^24 beside its neighbours (the widening is exact: distinct bit patterns stay distinct)
        (abi.F32, [None, 0.0, -0.0, _f32(0x7fc00001), _f32(0x7fc00002), _f32(0x4b800000), _f32(0x4b800001), _f32(0x4b7fffff), 0.1]),
        (abi.BYTES, [None, b"", b"a", b"ab", b"abc", b"abcdefgh", b"abcdefghi", b"abcdefgh\0", b"\0", b"\0\0", b"abcdefgX", b"abcdefghiJ", b"abcdefghiK"]),
    ]


def _stored_hex(tp, v):
    if v is None:
        return "-" if tp == abi.BYTES else ("00" * (4 if tp == abi.F32 else 8))
    if tp == abi.BYTES:
        return v.hex() or "-"
    fmt = {abi.I64: "<q", abi.U64: "<Q", abi.F32: "<f", abi.F64: "<d"}[tp]
    return struct.pack(fmt, v).hex()


def test_cell_images_agree_with_the_oracle_group_key_encoding(tmp_path, orc):
    exe = tmp_path / "groupid_cells"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "groupid_cells_main.cpp"), "-o", str(exe)], check=True)
    lines, want = [], []
    for tp, cells in cell_table():
        col = StrColumn(cells) if tp == abi.BYTES else Column(tp, [0 if v is None else v for v in cells], [v is not None for v in cells])
        enc = [R.encode_cell(orc, col, r) for r in range(len(cells))]
        for i, a in enumerate(cells):
            for j, b in enumerate(cells):
                lines.append("%d %d %s %d %s" % (tp, a is None, _stored_hex(tp, a), b is None, _stored_hex(tp, b)))
                want.append(1 if enc[i] == enc[j] else 0)
    # NULL against 0 and "" across the table above; the oracle itself must tell them apart
    assert R.encode_cell(orc, Column(abi.I64, [0], [False]), 0) != R.encode_cell(orc, Column(abi.I64, [0]), 0)
    assert R.encode_cell(orc, StrColumn([None]), 0) != R.encode_cell(orc, StrColumn([b""]), 0)
    res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
    got = [int(x) for x in res.stdout.split()]
    assert len(got) == len(want)
    bad = [(lines[i], want[i], got[i]) for i in range(len(want)) if want[i] != got[i]]
    assert not bad, bad[:10]
    assert 0 in want and 1 in want


def test_numpy_restatement_of_the_encoding_agrees_with_the_oracle_on_the_cell_table(orc):
    for tp, cells in cell_table():
        col = StrColumn(cells) if tp == abi.BYTES else Column(tp, [0 if v is None else v for v in cells], [v is not None for v in cells])
        assert np.array_equal(R.np_ids([col]), R.oracle_ids(orc, [col])), tp
