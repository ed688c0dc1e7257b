"""CPU: (a) tests/cast_ref.py — the restatement the GPU tests of the INSERT .. SELECT step compare with — against the vectors of the
reference's own tests (tests/golden/cast_cases.json); (b) the per-cell code of the kernels (tinysql_amd/csrc/tsq_insert_dp.h, built
on the host as a stand-alone sanitized program, tests/insert_dp_main.cpp) against cast_ref on an edge grid and on 1e5 fuzzed cells
per (source, target) pair; (c) the auto-id operator under random bracketing against the sequential loop; (d) the C-ABI."""
import json
import math
import os
import random
import re
import struct
import subprocess

import pytest

from tests import cast_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
GOLD = json.load(open(os.path.join(ROOT, "tests", "golden", "cast_cases.json")))
TP = {"tiny": abi.TP_TINY, "short": abi.TP_SHORT, "int24": abi.TP_INT24, "long": abi.TP_LONG, "longlong": abi.TP_LONGLONG, "float": abi.TP_FLOAT,
      "double": abi.TP_DOUBLE, "blob": abi.TP_BLOB, "string": abi.TP_STRING, "varchar": abi.TP_VARCHAR}
SRC = {"i64": abi.I64, "u64": abi.U64, "f32": abi.F32, "f64": abi.F64, "bytes": abi.BYTES}
STMT = {"IGNORE_TRUNCATE": abi.CAST_IGNORE_TRUNCATE, "TRUNCATE_AS_WARNING": abi.CAST_TRUNCATE_AS_WARNING, "IN_INSERT": abi.CAST_IN_INSERT}
U64 = (1 << 64) - 1


# ---------------------------------------------------------------- (a) cast_ref against the reference's vectors
@pytest.mark.parametrize("case", GOLD["convert"], ids=lambda c: c["ref"])
def test_ref_convert_vectors(case):
    sc = R.StmtCtx(sum(STMT[s] for s in case["stmt"]))
    v = case["v"]
    if case["src"] == "f32":
        v = R.to_f32(v)
    ft = R.FieldType(TP[case["tp"]], case["flen"], case["decimal"], case["unsigned"], charset=case.get("charset", ""))
    if case["src"] == "bytes" and ft.tp in R.INT_BITS:  # (types.Convert: a zero StatementContext, CastStrToIntStrict false)
        got, err = R.convert_to(R.StmtCtx(0, abi.STRCTX_NOT_STRICT | abi.STRCTX_EMPTY_NOT_ZERO | abi.STRCTX_TRUNCATE_ERROR), abi.BYTES, v.encode(), ft)
        assert (got, err) == (case["want"], None), case["ref"]
        return
    if case["src"] == "bytes":  # (ErrDataTooLong comes back from ProduceStrWithSpecifiedTp's own HandleTruncate: a strict context)
        got, err = R.convert_to(sc, abi.BYTES, v.encode(), ft)
        assert got == case["want"].encode() and (err == abi.ERR_DATA_TOO_LONG) == case["err"], case["ref"]
        return
    got, err = R.convert_to(sc, SRC[case["src"]], v, ft)  # types.Convert: ConvertTo alone, the error as it is
    want = case["want"]
    if want == "widened_input":
        want = v
    elif case["want_is_float32_literal"]:
        want = R.to_f32(want)
    assert got == want and isinstance(got, int) == isinstance(want, int), case["ref"]
    assert (err is not None) == case["err"], case["ref"]


def test_ref_round_float_round_truncate_vectors():
    for c in GOLD["round_float"]:
        assert R.round_float(float(c["in"])) == c["want"], c["ref"]
    for c in GOLD["round"]:
        assert R.go_round(c["in"], c["dec"]) == c["want"], c["ref"]
    for c in GOLD["truncate_float"]:
        assert R.truncate_float(c["in"], c["flen"], c["decimal"]) == (c["want"], c["overflow"]), c["ref"]


def test_ref_handle_bad_null_and_zero_values():
    for c in GOLD["handle_bad_null"]:
        cols = [R.FieldType(abi.TP_LONG, not_null=c["not_null"])]
        flags = abi.CAST_BAD_NULL_AS_WARNING if c["bad_null_as_warning"] else 0
        if c["error"]:
            with pytest.raises(R.CastError) as e:
                R.cast_rows(flags, [[None]], [abi.I64], cols, [0])
            assert (e.value.row, e.value.col, e.value.code) == (0, 0, abi.ERR_BAD_NULL)
        else:
            rows, sc = R.cast_rows(flags, [[None]], [abi.I64], cols, [0])
            assert (rows[0][0] is None) == c["want_null"], c["ref"]
            assert sc.warn_bad_null == (1 if c["bad_null_as_warning"] and c["not_null"] else 0)
    for c in GOLD["zero_value"]:
        z = R.zero_value(R.FieldType(TP[c["tp"]], unsigned=c["unsigned"]))
        assert z == c["want"] and type(z) is type(c["want"]), c["ref"]


@pytest.mark.parametrize("case", GOLD["auto_id"], ids=lambda c: c["ref"])
def test_ref_auto_id_vectors(case):
    ids, nb, first, last = R.fill_auto_ids(case["in"], case["base"], case["no_auto_value_on_zero"], case["upper"])
    assert (ids, nb, first, last) == (case["want"], case["new_base"], case["first_allocated"], case["last_explicit"])


def test_ref_error_order_is_row_then_casts_then_not_null():
    # table (a TINYINT NOT NULL, b TINYINT, c TINYINT); the statement names (c, b, a) in that order: src_cols = [2, 1, 0]
    cols = [R.FieldType(abi.TP_TINY, not_null=True), R.FieldType(abi.TP_TINY), R.FieldType(abi.TP_TINY)]
    with pytest.raises(R.CastError) as e:  # row 0: vals[0] -> c overflows, vals[1] -> b overflows: the statement's first column wins
        R.cast_rows(0, [[300, 300, 1]], [abi.I64] * 3, cols, [2, 1, 0])
    assert (e.value.row, e.value.col, e.value.code) == (0, 2, abi.ERR_OUT_OF_RANGE)
    with pytest.raises(R.CastError) as e:  # a NULL for `a` and an overflow for `b` in one row: the cast loop runs first
        R.cast_rows(0, [[1, 300, None]], [abi.I64] * 3, cols, [2, 1, 0])
    assert (e.value.row, e.value.col, e.value.code) == (0, 1, abi.ERR_OUT_OF_RANGE)
    with pytest.raises(R.CastError) as e:  # an earlier row's NOT NULL failure beats a later row's overflow
        R.cast_rows(0, [[1, 1, None], [300, 1, 1]], [abi.I64] * 3, cols, [2, 1, 0])
    assert (e.value.row, e.value.col, e.value.code) == (0, 0, abi.ERR_BAD_NULL)


# ---------------------------------------------------------------- (b) the kernels' per-cell code against cast_ref
@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("insert") / "insert_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all", "-ffp-contract=off",
                    os.path.join(ROOT, "tests", "insert_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
        out = res.stdout.splitlines()
        assert len(out) == len(lines)
        return [ln.split() for ln in out]
    return run


def f64_bits(f):
    return struct.unpack("<Q", struct.pack("<d", f))[0]


def bits_f64(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def f32_bits(f):
    """f is float32-representable (or inf / NaN)"""
    return struct.unpack("<I", struct.pack("<f", f))[0]


def bits_f32(b):
    return struct.unpack("<f", struct.pack("<I", b & 0xffffffff))[0]


def cell_bits(src_type, v):
    if src_type == abi.I64:
        return v & U64
    if src_type == abi.U64:
        return v
    return f32_bits(v) if src_type == abi.F32 else f64_bits(v)


def out_bits(ft, v):
    if ft.tp in R.INT_BITS:
        return v & U64
    return f32_bits(v) if ft.tp == abi.TP_FLOAT else f64_bits(v)


def same_cell(ft, got_bits, want):
    """want: the reference's value.  A NaN passes through a float column without (M, D): any NaN is "the" NaN"""
    if isinstance(want, float) and want != want:
        return math.isnan(bits_f32(got_bits) if ft.tp == abi.TP_FLOAT else bits_f64(got_bits))
    return got_bits == out_bits(ft, want)


TARGETS = [R.FieldType(tp, unsigned=u) for tp in (abi.TP_TINY, abi.TP_SHORT, abi.TP_INT24, abi.TP_LONG, abi.TP_LONGLONG) for u in (False, True)]
REALS = [R.FieldType(abi.TP_FLOAT), R.FieldType(abi.TP_DOUBLE), R.FieldType(abi.TP_FLOAT, 5, 2), R.FieldType(abi.TP_DOUBLE, 10, 0), R.FieldType(abi.TP_DOUBLE, 8, 2),
         R.FieldType(abi.TP_DOUBLE, 8, 2, unsigned=True), R.FieldType(abi.TP_FLOAT, 12, 4), R.FieldType(abi.TP_DOUBLE, 40, 8), R.FieldType(abi.TP_DOUBLE, 255, 30),
         R.FieldType(abi.TP_DOUBLE, unsigned=True)]
STMT_SETS = [0, abi.CAST_IN_INSERT, abi.CAST_IN_INSERT | abi.CAST_TRUNCATE_AS_WARNING, abi.CAST_IGNORE_TRUNCATE, abi.CAST_OVERFLOW_AS_WARNING,
             abi.CAST_OVERFLOW_AS_WARNING | abi.CAST_TRUNCATE_AS_WARNING | abi.CAST_IN_INSERT]


def nextafter32(f, up):
    b = f32_bits(f)
    if f == 0:
        return bits_f32(1 if up else 0x80000001)
    return bits_f32(b + 1 if (f > 0) == up else b - 1)


def edge_values(src_type):
    ints = set()
    for b in (8, 16, 24, 32, 64):
        for e in (-(1 << (b - 1)), (1 << (b - 1)) - 1, (1 << b) - 1, 0):
            ints.update((e - 1, e, e + 1))
    if src_type == abi.I64:
        return sorted(v for v in ints if R.I64MIN <= v <= R.I64MAX)
    if src_type == abi.U64:
        return sorted(v for v in ints if 0 <= v <= R.U64MAX)
    fl = {0.0, -0.0, 0.5, -0.5, 1.5, -1.5, 2.5, -2.5, 0.49999999999999994, -0.49999999999999994, 2.0 ** 63, -2.0 ** 63, 2.0 ** 64, math.inf, -math.inf, math.nan,
          math.nextafter(2.0 ** 63, 0), math.nextafter(2.0 ** 63, math.inf), math.nextafter(-2.0 ** 63, -math.inf), math.nextafter(2.0 ** 64, 0), 1e300, -1e300, 5e-324,
          999.99, 999.994, 999.995, 999.9949999, 1000.0, -999.995, 99999999.5, 9999999999.0, 9999999999.4, 9999999999.5, 999999.99, 999999.994, 999999.995, 1e38, 3.5e38, 1e39}
    for v in ints:
        for d in (-1.0, -0.5, -0.49, 0.0, 0.49, 0.5, 1.0):
            fl.add(float(v) + d)
    if src_type == abi.F64:
        return sorted(fl, key=lambda x: (x != x, x))
    f32 = set()
    for f in fl:
        g = R.to_f32(f)
        f32.add(g)
        if g == g and not math.isinf(g):
            f32.update((nextafter32(g, True), nextafter32(g, False)))
    return sorted(f32, key=lambda x: (x != x, x))


def check_cells(dp, src_type, ft, stmt, cells):
    """cells: python values or None.  The program's answers against cast_ref, cell by cell"""
    lines = ["col 0 %d %d %d %d %d %d 0" % (src_type, ft.tp, ft.flen, ft.decimal, ft.flags(), stmt)]
    lines += ["x %d %x" % ((1, 0) if v is None else (0, cell_bits(src_type, v))) for v in cells]
    got = dp(lines)
    assert got[0] == ["0"]
    for v, g in zip(cells, got[1:]):
        sc = R.StmtCtx(stmt)
        status, phase, onull, bits, w_ovf, w_null = int(g[0]), int(g[1]), int(g[2]), int(g[3], 16), int(g[4]), int(g[5])
        try:
            row = R.get_row(sc, 0, [v], [src_type], [ft], [0])
        except R.CastError as e:
            assert (status, phase) == (e.code, 1 if e.code == abi.ERR_BAD_NULL else 0), (src_type, ft.tp, ft.unsigned, stmt, v, g)
            continue
        assert status == 0, (src_type, ft.tp, ft.unsigned, ft.flen, ft.decimal, stmt, v, g)
        assert (w_ovf, w_null) == (sc.warn_overflow, sc.warn_bad_null), (src_type, ft.tp, ft.unsigned, ft.flen, ft.decimal, stmt, v, g)
        assert onull == (1 if row[0] is None else 0), (src_type, ft.tp, stmt, v, g)
        if row[0] is not None:
            assert same_cell(ft, bits, row[0]), (src_type, ft.tp, ft.unsigned, ft.flen, ft.decimal, stmt, v, g, row[0])


@pytest.mark.parametrize("src_type", [abi.I64, abi.U64, abi.F32, abi.F64], ids=["i64", "u64", "f32", "f64"])
def test_edge_grid_equals_cast_ref(dp, src_type):
    cells = edge_values(src_type) + [None]
    for ft in TARGETS + REALS:
        for stmt in STMT_SETS:
            check_cells(dp, src_type, ft, stmt, cells)
        nn = R.FieldType(ft.tp, ft.flen, ft.decimal, ft.unsigned, not_null=True)
        check_cells(dp, src_type, nn, 0, [None, cells[0]])
        check_cells(dp, src_type, nn, abi.CAST_BAD_NULL_AS_WARNING, [None, cells[0]])


def fuzz_cells(rng, src_type, n):
    out = []
    for _ in range(n):
        k = rng.randrange(8)
        if src_type in (abi.I64, abi.U64):
            if k < 3:
                v = rng.getrandbits(64)
            elif k < 6:
                b = rng.choice((8, 16, 24, 32, 64))
                v = rng.choice((1 << (b - 1), (1 << b), 0)) + rng.randrange(-3, 4)
                if rng.random() < 0.5:
                    v = -v
            else:
                v = rng.getrandbits(rng.randrange(1, 64))
            v &= U64
            out.append(v - (1 << 64) if src_type == abi.I64 and v >> 63 else v)
        else:
            if k < 2:
                v = bits_f64(rng.getrandbits(64)) if src_type == abi.F64 else bits_f32(rng.getrandbits(32))
            elif k < 5:
                b = rng.choice((8, 16, 24, 32, 63, 64))
                v = float(rng.choice((1 << (b - 1), 1 << b))) * rng.choice((1, -1)) + rng.choice((-1.5, -1, -0.5, -0.25, 0, 0.25, 0.5, 1, 1.5)) * rng.choice((1, 1 + 2 ** -40))
            elif k < 7:
                v = round(rng.uniform(-2e6, 2e6), rng.randrange(0, 6))
            else:
                v = rng.uniform(-1, 1) * 10 ** rng.randrange(-3, 40)
            out.append(R.to_f32(v) if src_type == abi.F32 else v)
    return out


@pytest.mark.parametrize("src_type", [abi.I64, abi.U64, abi.F32, abi.F64], ids=["i64", "u64", "f32", "f64"])
def test_fuzzed_cells_equal_cast_ref(dp, src_type):
    """1e5 cells per (source, target) pair: the ten integer targets and FLOAT / DOUBLE, (M, D) forms drawn among the cells"""
    rng = random.Random(1000 + src_type)
    n, piece = 100000, 12500
    reals = {abi.TP_FLOAT: [f for f in REALS if f.tp == abi.TP_FLOAT], abi.TP_DOUBLE: [f for f in REALS if f.tp == abi.TP_DOUBLE]}
    for ft in TARGETS + [abi.TP_FLOAT, abi.TP_DOUBLE]:
        for i in range(n // piece):
            f = ft if isinstance(ft, R.FieldType) else reals[ft][i % len(reals[ft])]
            check_cells(dp, src_type, f, STMT_SETS[i % len(STMT_SETS)], fuzz_cells(rng, src_type, piece))


def test_pow10_is_gos_table_product(dp):
    ns = list(range(-330, 315))
    got = dp(["p %d" % n for n in ns])
    for n, g in zip(ns, got):
        assert int(g[0], 16) == f64_bits(R.pow10(n)), n
    # where the product of two table entries is NOT the correctly rounded power, Go's value is the product
    assert any(R.pow10(n) != float("1e%d" % n) for n in range(33, 309))


def test_defaults_and_unsupported_columns(dp):
    lines = ["col -1 0 %d -1 -1 0 0 %x" % (abi.TP_LONG, 42), "x 0 7", "col -1 0 %d -1 -1 %d 0 0" % (abi.TP_LONG, abi.CAST_DEFAULT_NULL), "x 0 7",
             "col -1 0 %d -1 -1 %d 0 0" % (abi.TP_LONG, abi.CAST_DEFAULT_NULL | abi.CAST_NOT_NULL), "x 0 7",
             "col -1 0 %d -1 -1 %d 0 5" % (abi.TP_LONGLONG, abi.CAST_AUTO_INCREMENT | abi.CAST_NOT_NULL), "x 0 7"]
    got = dp(lines)
    assert got[1] == ["0", "0", "0", "2a", "0", "0"]          # the default
    assert got[3][:3] == ["0", "0", "1"]                      # DEFAULT NULL
    assert got[5][:2] == [str(abi.ERR_BAD_NULL), "1"]         # ... in a NOT NULL column
    assert got[7][:3] == ["0", "0", "1"]                      # an auto-increment column nobody named: NULL, exempt from the check
    unsupported = [(0, abi.BYTES, abi.TP_DOUBLE, 0), (0, abi.BYTES, abi.TP_FLOAT, 0), (0, abi.F64, abi.TP_VARCHAR, 0), (0, abi.I64, abi.TP_BIT, 0),
                   (0, abi.I64, abi.TP_LONGLONG, abi.CAST_AUTO_INCREMENT | abi.CAST_UNSIGNED), (0, abi.F64, abi.TP_DOUBLE, abi.CAST_AUTO_INCREMENT)]
    got = dp(["col %d %d %d -1 -1 %d 0 0" % u for u in unsupported])
    assert all(g == [str(abi.ERR_UNSUPPORTED)] for g in got)
    assert dp(["col 0 0 6 -1 -1 0 0 0"]) == [[str(abi.ERR_INVALID)]]  # TypeNull is no column type


# ---- string sources into integer columns
def test_ref_str_to_num_vectors():
    from tests import strtoint_ref as S
    loose = abi.STRCTX_NOT_STRICT | abi.STRCTX_EMPTY_NOT_ZERO  # testStrToInt / testStrToUint: a zero context + IgnoreTruncate = !truncateAsErr
    for name, fn in (("str_to_int", S.str_to_int), ("str_to_uint", R.str_to_uint)):
        for c in GOLD[name]:
            v, f = fn(c["in"].encode(), loose | (abi.STRCTX_TRUNCATE_ERROR if c["truncate_as_err"] else abi.STRCTX_IGNORE_TRUNCATE))
            err = "overflow" if f & S.ERR_OVF else "truncated" if f & S.ERR_TRUNC else None
            assert err == c["err"] and (c["err"] is not None or v == c["want"]), c["ref"]
    for c in GOLD["get_valid_int"]:  # CastStrToIntStrict, TruncateAsWarning: str_ctx 0; the prefix must parse and a cut is a warning
        v, f = (S.str_to_int if c["signed"] else R.str_to_uint)(c["in"].encode(), 0)
        assert v == int(c["valid"]) and bool(f & S.TRUNC_WARN) == c["warning"] and not f & (S.ERR_OVF | S.ERR_TRUNC), c["ref"]


STR_CTXS = [0, 1, 2, 4, 8 | 1, 8 | 1 | 2, 8 | 1 | 4, 2 | 1]
INT_STRINGS = [b"", b" ", b"0", b"-0", b"+0", b"1", b"-1", b"+1", b"+", b"-", b"+-1", b"127", b"128", b"-128", b"-129", b"255", b"256", b"65535", b"65536", b"8388607", b"8388608",
               b"-8388609", b"16777215", b"16777216", b"2147483647", b"2147483648", b"-2147483649", b"4294967295", b"4294967296", b"9223372036854775807", b"9223372036854775808",
               b"-9223372036854775808", b"-9223372036854775809", b"18446744073709551615", b"18446744073709551616", b"99999999999999999999999", b"-99999999999999999999999",
               b"1.4", b"1.5", b"-1.5", b"0.5", b"-0.5", b".5", b"1.", b"1e2", b"1e-1", b"12e1", b"1.5e3", b"9.9e18", b"1e19", b"1.9e19", b"2e19", b"1e20", b"1e30", b"-1e19",
               b"254.5", b"255.4", b"255.5", b"127.5", b" 12 ", b"\t12\n", b"12abc", b"abc", b"1 2", b"0x10", b"+12", b"++12", b"--12", b"1e", b"1e+", b"e5", b"\xff12", b"12\xff",
               "\u00a012".encode(), b"00000000000000000000000000012", b"18446744073709551615.5", b"9223372036854775807.5"]


def check_str_int_cells(dp, ft, stmt, str_ctx, cells):
    lines = ["col 0 %d %d -1 -1 %d %d 0 %d" % (abi.BYTES, ft.tp, ft.flags(), stmt, str_ctx)]
    lines += ["z %d %s" % ((1, "-") if v is None else (0, v.hex() or "-")) for v in cells]
    got = dp(lines)
    assert got[0] == ["0"]
    for v, g in zip(cells, got[1:]):
        sc = R.StmtCtx(stmt, str_ctx)
        status, phase, onull, bits = int(g[0]), int(g[1]), int(g[2]), int(g[3], 16)
        where = (ft.tp, ft.unsigned, ft.not_null, stmt, str_ctx, v, g)
        try:
            row = R.get_row(sc, 0, [v], [abi.BYTES], [ft], [0])
        except R.CastError as e:
            assert (status, phase) == (e.code, 1 if e.code == abi.ERR_BAD_NULL else 0), where
            continue
        assert status == 0, where
        assert [int(x) for x in g[4:7]] == [sc.warn_overflow, sc.warn_bad_null, sc.warn_truncated], where
        assert onull == (1 if row[0] is None else 0) and (row[0] is None or bits == row[0] & U64), where + (row[0],)


def test_string_to_integer_edge_grid_equals_cast_ref(dp):
    """every integer type's bounds +-1 as strings, signs, float prefixes and exponents, garbage — under every statement / string context"""
    for ft in TARGETS:
        for stmt in STMT_SETS[:4]:
            for sctx in STR_CTXS:
                check_str_int_cells(dp, ft, stmt, sctx, INT_STRINGS + [None])
        nn = R.FieldType(ft.tp, unsigned=ft.unsigned, not_null=True)
        for stmt in (abi.CAST_IGNORE_TRUNCATE, abi.CAST_IGNORE_TRUNCATE | abi.CAST_BAD_NULL_AS_WARNING, abi.CAST_TRUNCATE_AS_WARNING | abi.CAST_BAD_NULL_AS_WARNING):
            check_str_int_cells(dp, nn, stmt, R.default_str_ctx(stmt), [None, b"300", b"-1", b"99999999999999999999", b"7"])  # the unsigned arm's NULLs meet NOT NULL


def test_fuzzed_string_to_integer_cells_equal_cast_ref(dp):
    """1e5 cells for the pair (string, integer column): the ten integer targets, the contexts changing every 2500 cells"""
    rng = random.Random(77)
    alphabet = b"0123456789" * 3 + b"+-.eE  x"
    for i in range(40):
        ft = TARGETS[i % len(TARGETS)]
        cells = []
        for _ in range(2500):
            k = rng.randrange(5)
            if k == 0:
                cells.append(bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 24))))
            elif k == 1:
                cells.append(str(rng.getrandbits(rng.randrange(1, 70)) * rng.choice((1, -1))).encode())
            elif k == 2:
                cells.append(("%s%d.%d" % (rng.choice(("", "-", "+")), rng.getrandbits(rng.randrange(1, 66)), rng.randrange(0, 100))).encode())
            elif k == 3:
                cells.append(("%d.%de%d" % (rng.randrange(0, 1000), rng.randrange(0, 1000), rng.randrange(-5, 25))).encode())
            else:
                cells.append(rng.choice(INT_STRINGS) + bytes(rng.choice(alphabet) for _ in range(rng.randrange(0, 3))))
        stmt = STMT_SETS[i % 4]
        check_str_int_cells(dp, ft, stmt, rng.choice(STR_CTXS + [R.default_str_ctx(stmt)] * 4), cells)


# ---- string targets
STR_PIECES = [b"a", b"Z", b" ", "\u00e9".encode(), "\u20ac".encode(), "\U0001F600".encode(), b"\xef\xbf\xbd", b"\xff", b"\xe2\x82", b"\xed\xa0\x80", b"\xc0\xaf", b"\xf4\x90\x80\x80", b"0"]
STR_TARGETS = [R.FieldType(tp, flen, charset=cs) for tp in (abi.TP_VARCHAR, abi.TP_STRING, abi.TP_BLOB, abi.TP_VAR_STRING, abi.TP_TINY_BLOB) for flen in (-1, 0, 1, 3, 5)
               for cs in ("utf8", "utf8mb4", "binary", "")]
STR_STMTS = [0, abi.CAST_TRUNCATE_AS_WARNING, abi.CAST_IGNORE_TRUNCATE, abi.CAST_SKIP_UTF8_CHECK, abi.CAST_TRUNCATE_AS_WARNING | abi.CAST_SKIP_UTF8_CHECK]


def check_str_cells(dp, src_type, ft, stmt, cells):
    lines = ["col 0 %d %d %d -1 %d %d 0" % (src_type, ft.tp, ft.flen, ft.flags(), stmt)]
    lines += [("y %d %s" % ((1, "-") if v is None else (0, v.hex() or "-"))) if src_type == abi.BYTES else ("x %d %x" % ((1, 0) if v is None else (0, v & U64))) for v in cells]
    got = dp(lines)
    assert got[0] == ["0"]
    for v, g in zip(cells, got[1:]):
        sc = R.StmtCtx(stmt)
        status, phase, onull, cell = int(g[0]), int(g[1]), int(g[2]), (b"" if g[3] == "-" else bytes.fromhex(g[3]))
        where = (src_type, ft.tp, ft.flen, ft.charset, ft.not_null, stmt, v, g)
        try:
            row = R.get_row(sc, 0, [v], [src_type], [ft], [0])
        except R.CastError as e:
            assert (status, phase) == (e.code, 1 if e.code == abi.ERR_BAD_NULL else 0), where
            continue
        assert status == 0, where
        assert [int(x) for x in g[4:7]] == [sc.warn_bad_null, sc.warn_too_long, sc.warn_bad_utf8], where
        assert onull == (1 if row[0] is None else 0) and (row[0] is None or cell == row[0]), where + (row[0],)


def edge_strings():
    """strings of 0 .. Flen + 1 runes (Flen up to 5) from 1- to 4-byte runes, invalid bytes, a literal U+FFFD, spaces in front and behind"""
    out = [b"", b" ", b"  ", b"a ", b" a", b"a  ", b"\xef\xbf\xbd", b"a\xef\xbf\xbd ", b"\xff", b"ab\xffcd", "\U0001F600".encode(), ("a" + "\U0001F600").encode()]
    rng = random.Random(3)
    for n in range(0, 7):
        for _ in range(40):
            out.append(b"".join(rng.choice(STR_PIECES) for _ in range(n)) + b" " * rng.choice((0, 0, 1, 2)))
    return out


def test_string_edge_grid_equals_cast_ref(dp):
    cells = edge_strings() + [None]
    for ft in STR_TARGETS:
        for stmt in STR_STMTS:
            check_str_cells(dp, abi.BYTES, ft, stmt, cells)
        nn = R.FieldType(ft.tp, ft.flen, charset=ft.charset, not_null=True)
        check_str_cells(dp, abi.BYTES, nn, 0, [None, b"x"])
        check_str_cells(dp, abi.BYTES, nn, abi.CAST_BAD_NULL_AS_WARNING, [None, b"x"])
    ints = [0, 1, -1, 9, 10, -9, -10, 99999, 100000, -99999, R.I64MAX, R.I64MIN, None]
    for ft in STR_TARGETS + [R.FieldType(abi.TP_STRING, 24, charset="binary"), R.FieldType(abi.TP_VARCHAR, 20, charset="utf8")]:
        for stmt in STR_STMTS[:3]:
            check_str_cells(dp, abi.I64, ft, stmt, ints)
            check_str_cells(dp, abi.U64, ft, stmt, [0, 7, 10, R.U64MAX, 1 << 63, 12345678901234567890, None])


@pytest.mark.parametrize("src_type", [abi.BYTES, abi.I64, abi.U64], ids=["bytes", "i64", "u64"])
def test_fuzzed_string_cells_equal_cast_ref(dp, src_type):
    """1e5 cells per source into the string family, the target and the statement flags changing every 2500 cells"""
    rng = random.Random(2000 + src_type)
    for i in range(40):
        ft = STR_TARGETS[rng.randrange(len(STR_TARGETS))]
        if rng.random() < 0.3:
            ft = R.FieldType(ft.tp, rng.randrange(0, 30), charset=ft.charset)
        if src_type == abi.BYTES:
            cells = [b"".join(rng.choice(STR_PIECES) for _ in range(rng.randrange(0, 12))) + b" " * rng.choice((0, 0, 0, 1, 3)) if rng.random() < 0.8
                     else bytes(rng.getrandbits(8) for _ in range(rng.randrange(0, 16))) for _ in range(2500)]
        else:
            cells = [rng.getrandbits(rng.randrange(1, 65)) * (rng.choice((1, -1)) if src_type == abi.I64 else 1) for _ in range(2500)]
            cells = [max(R.I64MIN, min(R.I64MAX, v)) if src_type == abi.I64 else v for v in cells]
        check_str_cells(dp, src_type, ft, STR_STMTS[i % len(STR_STMTS)], cells)


# ---------------------------------------------------------------- (c) the auto-id operator
def test_auto_id_operator_under_random_bracketing_equals_the_sequential_loop(dp):
    rng = random.Random(7)
    lines, wants = [], []
    for t in range(10000):
        n = rng.randrange(0, 71)
        mode = rng.randrange(5)
        upper = rng.choice((127, 32767, (1 << 31) - 1, R.I64MAX))
        top = {0: 50, 1: upper, 2: R.I64MAX, 3: 200, 4: 10}[mode]
        base = rng.choice((0, rng.randrange(0, 100), max(0, top - rng.randrange(0, 80))))
        vals = []
        for _ in range(n):
            k = rng.random()
            if k < 0.4:
                vals.append(None)
            elif k < 0.5:
                vals.append(0)
            elif k < 0.6:
                vals.append(-rng.randrange(1, 1 << rng.randrange(1, 63)))
            else:
                vals.append(max(1, min(upper, top - rng.randrange(0, 90))) if rng.random() < 0.7 else rng.randrange(1, 100))
        flags = rng.randrange(2)
        lines.append("a %d %d %d %d %d %s" % (base, flags, upper, rng.getrandbits(63), n, " ".join("N" if v is None else str(v) for v in vals)))
        try:
            wants.append(R.fill_auto_ids(vals, base, bool(flags), upper))
        except R.AutoIdError as e:
            wants.append(e)
    got = dp(lines)
    kinds = {"ok": 0, abi.ERR_OUT_OF_RANGE: 0, abi.ERR_UNSUPPORTED: 0}
    for ln, g, w in zip(lines, got, wants):
        ovf, nb, bad, ids = int(g[0]), int(g[1]), int(g[2]), [int(x) for x in g[3:]]
        if isinstance(w, R.AutoIdError):
            kinds[w.code] += 1
            if w.code == abi.ERR_OUT_OF_RANGE:
                assert bad == w.row, ln
            else:
                assert ovf == 1 and bad == -1, ln
            continue
        kinds["ok"] += 1
        assert (ovf, bad, ids, nb) == (0, -1, w[0], w[1]), ln
    assert min(kinds.values()) > 50, kinds  # every outcome is exercised


# ---------------------------------------------------------------- (d) the C-ABI
NAMES = ["tsq_cast_create", "tsq_cast_run", "tsq_cast_error_at", "tsq_cast_warnings", "tsq_cast_stats", "tsq_cast_cancel", "tsq_cast_destroy", "tsq_autoid_fill"]


def test_new_abi_is_declared_exported_and_the_version_stays():
    assert abi.TSQ_ABI_VERSION == 10
    lib = _lib.load()
    hdr = open(os.path.join(ROOT, "include", "tsq.h")).read()
    for name in NAMES:
        assert name in abi.SIGNATURES and hasattr(lib, name) and name + "(" in hdr, name
    assert lib.tsq_abi_version() == 10
    for name, val in (("DATA_TOO_LONG", 12), ("OUT_OF_RANGE", 13), ("BAD_NULL", 14), ("BAD_UTF8", 15)):
        assert re.search(r"TSQ_ERR_%s = %d\b" % (name, val), hdr) and getattr(abi, "ERR_" + name) == val and abi.STATUS_NAMES[val] == name
    assert re.search(r"TSQ_ERR_TRUNCATED_WRONG_VALUE = 11\b", hdr)
    for name in ("IGNORE_TRUNCATE", "TRUNCATE_AS_WARNING", "OVERFLOW_AS_WARNING", "BAD_NULL_AS_WARNING", "IN_INSERT", "SKIP_UTF8_CHECK", "UNSIGNED", "NOT_NULL",
                 "AUTO_INCREMENT", "CHARSET_BIN", "CHARSET_UTF8", "CHARSET_UTF8MB4", "DEFAULT_NULL"):
        assert re.search(r"#define TSQ_CAST_%s %du\b" % (name, getattr(abi, "CAST_" + name)), hdr), name
    for name in ("TINY", "SHORT", "LONG", "FLOAT", "DOUBLE", "LONGLONG", "INT24", "VARCHAR", "BIT", "TINY_BLOB", "MEDIUM_BLOB", "LONG_BLOB", "BLOB", "VAR_STRING", "STRING"):
        assert re.search(r"#define TSQ_TP_%s %d\b" % (name, getattr(abi, "TP_" + name)), hdr), name


def test_cast_col_layout_equals_what_gcc_computes(tmp_path):
    import ctypes as C
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu %%zu\\n", sizeof(tsq_cast_col), offsetof(tsq_cast_col, flags), '
                   'offsetof(tsq_cast_col, def_bits), offsetof(tsq_cast_col, def_len));return 0;}\n' % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.CastCol), abi.CastCol.flags.offset, abi.CastCol.def_bits.offset, abi.CastCol.def_len.offset]


def test_ctypes_prototypes_match_the_header():
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
