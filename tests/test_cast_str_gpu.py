"""GPU: the string targets of tsq_cast_run (Blob family, CHAR / BINARY, VARCHAR, VarString from string and integer sources) through the
C-ABI, byte for byte against tests/cast_ref.py, for host and device chunks: cells of 0, 1, 63, 64, 65 and 5000 bytes (the wave copy
starts at 64), Flen in runes and in bytes, BINARY padding, CHAR trimming, the UTF-8 walk, the sizing call that writes nothing,
defaults, the zero value of a NOT NULL string column, errors and warnings at their positions; and string sources into the integer
columns (StrToInt / StrToUint under the range clip)."""
import ctypes as C

import numpy as np
import pytest

from tests import cast_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import table as T
from tinysql_amd.chunk import Chunk, Column, StrColumn, make_cols, out_buffers
from tinysql_amd.gpu_pipeline import DeviceChunk

pytestmark = pytest.mark.gpu

PIECES = [b"a", b"Z", b" ", "é".encode(), "€".encode(), "\U0001F600".encode(), b"\xef\xbf\xbd", b"\xff", b"\xe2\x82", b"\xed\xa0\x80", b"\xc0\xaf", b"0"]


def info(ft):
    flag = (T.UnsignedFlag if ft.unsigned else 0) | (T.NotNullFlag if ft.not_null else 0)
    return T.ColumnInfo(ft.tp, ft.flen, ft.decimal, flag, DefaultValue=ft.default, Charset=ft.charset)


def stmt_of(flags):
    return T.StatementContext(IgnoreTruncate=bool(flags & abi.CAST_IGNORE_TRUNCATE), TruncateAsWarning=bool(flags & abi.CAST_TRUNCATE_AS_WARNING),
                              BadNullAsWarning=bool(flags & abi.CAST_BAD_NULL_AS_WARNING), InInsertStmt=bool(flags & abi.CAST_IN_INSERT),
                              SkipUTF8Check=bool(flags & abi.CAST_SKIP_UTF8_CHECK))


def run_cast(ctx, where, cols, fts, src_cols, flags):
    caster = T.Caster(ctx, [info(f) for f in fts], src_cols, [c.tp for c in cols], stmt_of(flags))
    try:
        if where == "host":
            return caster.run(Chunk(cols)), dict(caster.warnings)
        dchk = DeviceChunk.from_host(ctx, Chunk(cols))
        try:
            out = caster.run(dchk)
            try:
                return out.to_host(), dict(caster.warnings)
            finally:
                out.free()
        finally:
            dchk.free()
    finally:
        caster.close()


def rows_of(cols):
    return [list(r) for r in Chunk(cols).rows()]


def check(ctx, where, cols, fts, src_cols, flags):
    want, sc = R.cast_rows(flags, rows_of(cols), [c.tp for c in cols], fts, src_cols)
    got, warn = run_cast(ctx, where, cols, fts, src_cols, flags)
    assert got.rows() == [tuple(r) for r in want]
    assert (warn["data_too_long"], warn["bad_utf8"], warn["bad_null"], warn["overflow"]) == (sc.warn_too_long, sc.warn_bad_utf8, sc.warn_bad_null, sc.warn_overflow)
    return sc


def random_strings(rng, n, max_pieces, null_p):
    out = []
    for _ in range(n):
        if rng.random() < null_p:
            out.append(None)
            continue
        s = b"".join(PIECES[i] for i in rng.integers(0, len(PIECES), int(rng.integers(0, max_pieces + 1))))
        out.append(s + b" " * int(rng.integers(0, 3)) if rng.random() < 0.3 else s)
    return out


STR_TARGETS = [R.FieldType(abi.TP_VARCHAR, 8, charset="utf8mb4"), R.FieldType(abi.TP_STRING, 4, charset="utf8mb4"), R.FieldType(abi.TP_VARCHAR, 6, charset="utf8"),
               R.FieldType(abi.TP_STRING, 10, charset="binary"), R.FieldType(abi.TP_VAR_STRING, 5, charset="binary"), R.FieldType(abi.TP_BLOB, charset="binary"),
               R.FieldType(abi.TP_TINY_BLOB, 3, charset="utf8"), R.FieldType(abi.TP_MEDIUM_BLOB, 7), R.FieldType(abi.TP_LONG_BLOB, charset="utf8mb4"),
               R.FieldType(abi.TP_STRING, 0, charset="utf8"), R.FieldType(abi.TP_STRING, 6), R.FieldType(abi.TP_VARCHAR, 70, charset="utf8mb4")]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dens", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("n", [1, 63, 64, 65, 641])
def test_string_sources_into_every_string_target(ctx, n, dens, where):
    rng = np.random.default_rng(n + int(dens * 10))
    col = StrColumn(random_strings(rng, n, 12, dens))
    for flags in (abi.CAST_IN_INSERT | abi.CAST_TRUNCATE_AS_WARNING, abi.CAST_IGNORE_TRUNCATE, abi.CAST_TRUNCATE_AS_WARNING | abi.CAST_SKIP_UTF8_CHECK):
        sc = check(ctx, where, [col], STR_TARGETS, [0] * len(STR_TARGETS), flags)
        if n == 641 and dens == 0.0 and flags & abi.CAST_TRUNCATE_AS_WARNING:
            assert sc.warn_too_long > 100 and (sc.warn_bad_utf8 > 100 or flags & abi.CAST_SKIP_UTF8_CHECK)


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dens", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("st", [abi.I64, abi.U64], ids=["i64", "u64"])
def test_integer_sources_into_string_targets(ctx, st, dens, where):
    rng = np.random.default_rng(7 + st)
    n = 300
    edges = [0, 1, -1, 9, 10, -10, 99999, -99999, 1 << 31, (1 << 63) - 1, -(1 << 63), (1 << 64) - 1, 12345678901234567890]
    vals = [edges[rng.integers(0, len(edges))] if rng.random() < 0.5 else int(rng.integers(-(1 << 40), 1 << 40)) for _ in range(n)]
    lo, hi = (R.I64MIN, R.I64MAX) if st == abi.I64 else (0, R.U64MAX)
    vals = [min(max(v, lo), hi) for v in vals]
    nn = rng.random(n) >= dens if dens < 1.0 else np.zeros(n, bool)
    col = Column(st, np.array(vals, dtype=np.int64 if st == abi.I64 else np.uint64), nn)
    fts = [R.FieldType(abi.TP_VARCHAR, 5, charset="utf8mb4"), R.FieldType(abi.TP_STRING, 24, charset="binary"), R.FieldType(abi.TP_BLOB), R.FieldType(abi.TP_STRING, 3, charset="utf8"),
           R.FieldType(abi.TP_VARCHAR, 20, charset="utf8"), R.FieldType(abi.TP_STRING, 80, charset="binary")]
    for flags in (abi.CAST_TRUNCATE_AS_WARNING, abi.CAST_IGNORE_TRUNCATE):
        check(ctx, where, [col], fts, [0] * len(fts), flags)


@pytest.mark.parametrize("where", ["host", "device"])
def test_cells_of_0_1_63_64_65_and_5000_bytes(ctx, where):
    """the lane copies a cell below 64 bytes, the wave one from 64 on; BINARY(n) pads with the same two paths"""
    sizes = [0, 1, 63, 64, 65, 5000, 7, 64, 0, 129]
    vals = [bytes((i * 7 + k) % 251 for k in range(s)) for i, s in enumerate(sizes)] + [None, b"tail"]
    col = StrColumn(vals * 9)  # more than one wave step
    fts = [R.FieldType(abi.TP_BLOB, charset="binary"), R.FieldType(abi.TP_STRING, 64, charset="binary"), R.FieldType(abi.TP_STRING, 70, charset="binary"),
           R.FieldType(abi.TP_VAR_STRING, 64, charset="binary"), R.FieldType(abi.TP_STRING, 6000, charset="binary"), R.FieldType(abi.TP_LONG_BLOB, 5000)]
    check(ctx, where, [col], fts, [0] * len(fts), abi.CAST_TRUNCATE_AS_WARNING)
    text = ["", "x", "y" * 63, "z" * 64, "w" * 65, "é€" * 1000, "q" * 62 + "é", "\U0001F600" * 16]
    check(ctx, where, [StrColumn([t.encode() for t in text] * 10)], [R.FieldType(abi.TP_VARCHAR, 64, charset="utf8mb4"), R.FieldType(abi.TP_VARCHAR, 2000, charset="utf8"),
                                                                    R.FieldType(abi.TP_STRING, 63, charset="utf8mb4")], [0, 0, 0], abi.CAST_TRUNCATE_AS_WARNING)


def test_the_sizing_call_writes_nothing(ctx):
    vals = [b"abcdef", None, b"", b"xy " * 40]
    keep = []
    ins = make_cols([StrColumn(vals), Column(abi.I64, np.arange(4))], keep)
    caster = T.Caster(ctx, [T.ColumnInfo(abi.TP_VARCHAR, 200, Charset="utf8mb4"), T.ColumnInfo(abi.TP_LONG), T.ColumnInfo(abi.TP_STRING, 4, Charset="binary")], [0, 1, 1],
                      [abi.BYTES, abi.I64], T.StatementContext())
    try:
        types = [abi.BYTES, abi.I64, abi.BYTES]
        outs, bufs = out_buffers(types, 4, keep, var_bytes=[0, 0, 0])
        for b in bufs:
            for arr in b:
                arr[:] = 0x5a if arr.dtype == np.uint8 else 77
        before = [[arr.copy() for arr in b] for b in bufs]
        cap, need = (C.c_int64 * 3)(0, 0, 0), (C.c_int64 * 3)(-1, -1, -1)
        assert ctx.lib.tsq_cast_run(caster.h, ins, 2, 4, outs, cap, need) == abi.ERR_INVALID
        assert list(need) == [6 + 0 + 120, 0, 16]
        for b, b0 in zip(bufs, before):  # not a byte of any output column, the fixed-width one included
            for arr, arr0 in zip(b, b0):
                assert (arr == arr0).all()
        outs, bufs = out_buffers(types, 4, keep, var_bytes=[need[0] - 1, 0, need[2]])  # one byte short is still too small
        cap2 = (C.c_int64 * 3)(need[0] - 1, 0, need[2])
        assert ctx.lib.tsq_cast_run(caster.h, ins, 2, 4, outs, cap2, need) == abi.ERR_INVALID and need[0] == 126
        outs, bufs = out_buffers(types, 4, keep, var_bytes=[126, 0, 16])
        cap3 = (C.c_int64 * 3)(126, 0, 16)
        assert ctx.lib.tsq_cast_run(caster.h, ins, 2, 4, outs, cap3, need) == abi.OK
        assert bufs[0][2].tolist() == [0, 6, 6, 6, 126] and bufs[2][2].tolist() == [0, 4, 8, 12, 16]
        assert bytes(bufs[2][0][:16]) == b"0\0\0\0" b"1\0\0\0" b"2\0\0\0" b"3\0\0\0"
        assert ctx.lib.tsq_cast_run(caster.h, ins, 2, 4, outs, None, None) == abi.ERR_INVALID  # a string column needs the two arrays
    finally:
        caster.close()


@pytest.mark.parametrize("where", ["host", "device"])
def test_first_error_and_its_kind(ctx, where):
    n = 700
    base = [b"ok%d" % (i % 50) for i in range(n)]
    fts = [R.FieldType(abi.TP_VARCHAR, 5, charset="utf8mb4"), R.FieldType(abi.TP_STRING, 5, charset="utf8", not_null=True), R.FieldType(abi.TP_LONG)]
    ints = Column(abi.I64, np.arange(n))
    for row in (0, 63, 64, 511, 512, n - 1):
        for c, bad, code in ((0, "toolong".encode(), abi.ERR_DATA_TOO_LONG), (1, b"a\xffb", abi.ERR_BAD_UTF8), (1, "\U0001F600".encode(), abi.ERR_BAD_UTF8), (1, None, abi.ERR_BAD_NULL)):
            v = [list(base), list(base)]
            v[c][row] = bad
            cols = [StrColumn(v[0]), StrColumn(v[1]), ints]
            with pytest.raises(R.CastError) as w:
                R.cast_rows(abi.CAST_IN_INSERT, rows_of(cols), [abi.BYTES, abi.BYTES, abi.I64], fts, [0, 1, 2])
            assert (w.value.row, w.value.col, w.value.code) == (row, c, code)
            with pytest.raises(T.CastError) as e:
                run_cast(ctx, where, cols, fts, [0, 1, 2], abi.CAST_IN_INSERT)
            assert (e.value.row, e.value.column, e.value.status) == (row, c, code)
    # a numeric and a string error in one run: (row, statement column) order across the two kernels
    v0 = list(base)
    v0[300] = b"much too long"
    big = np.arange(n)
    big[299] = 1 << 40
    with pytest.raises(T.CastError) as e:
        run_cast(ctx, where, [StrColumn(v0), StrColumn(base), Column(abi.I64, big)], fts, [0, 1, 2], abi.CAST_IN_INSERT)
    assert (e.value.row, e.value.column, e.value.status) == (299, 2, abi.ERR_OUT_OF_RANGE)
    big[299], big[300] = 0, 1 << 40
    with pytest.raises(T.CastError) as e:
        run_cast(ctx, where, [StrColumn(v0), StrColumn(base), Column(abi.I64, big)], fts, [0, 1, 2], abi.CAST_IN_INSERT)
    assert (e.value.row, e.value.column, e.value.status) == (300, 0, abi.ERR_DATA_TOO_LONG)


@pytest.mark.parametrize("where", ["host", "device"])
def test_defaults_and_zero_values_of_string_columns(ctx, where):
    n = 200
    fts = [R.FieldType(abi.TP_LONG), R.FieldType(abi.TP_VARCHAR, 8, charset="utf8mb4", default=b"dflt"), R.FieldType(abi.TP_STRING, 6, charset="binary", default=b"ab\0\0\0\0"),
           R.FieldType(abi.TP_BLOB), R.FieldType(abi.TP_STRING, 3, charset="binary", not_null=True), R.FieldType(abi.TP_VARCHAR, 9, charset="utf8", not_null=True),
           R.FieldType(abi.TP_VARCHAR, 100, charset="utf8mb4", default=b"x" * 90)]
    infos = [info(f) for f in fts]
    infos[2].DefaultValue = b"ab"  # as the DDL keeps it: padded when the handle is made
    col = Column(abi.I64, np.arange(n))
    caster = T.Caster(ctx, infos, [0, -1, -1, -1, -1, -1, -1], [abi.I64], T.StatementContext(BadNullAsWarning=True))
    try:
        if where == "host":
            got = caster.run(Chunk([col]))
        else:
            d = DeviceChunk.from_host(ctx, Chunk([col]))
            try:
                o = caster.run(d)
                got = o.to_host()
                o.free()
            finally:
                d.free()
        assert caster.warnings["bad_null"] == 2 * n
    finally:
        caster.close()
    want, sc = R.cast_rows(abi.CAST_IN_INSERT | abi.CAST_BAD_NULL_AS_WARNING, [[i] for i in range(n)], [abi.I64], fts, [0, -1, -1, -1, -1, -1, -1])
    assert got.rows() == [tuple(r) for r in want] and want[7] == [7, b"dflt", b"ab\0\0\0\0", None, b"\0\0\0", b"", b"x" * 90]


# ---------------------------------------------------------------- string sources into integer columns
INT_TARGETS = [R.FieldType(tp, unsigned=u) for tp in (abi.TP_TINY, abi.TP_SHORT, abi.TP_INT24, abi.TP_LONG, abi.TP_LONGLONG) for u in (False, True)]
NUMBERS = [b"", b"0", b"-1", b"+1", b"127", b"128", b"-129", b"255", b"256", b"65536", b"8388608", b"16777216", b"2147483648", b"4294967296", b"9223372036854775807",
           b"9223372036854775808", b"18446744073709551615", b"18446744073709551616", b"-9223372036854775809", b"1.5", b"-0.5", b"1e3", b"1e20", b" 42 ", b"12abc", b"abc",
           b"+", b"3.99e2", b"255.5", b"00012", "\u00a07".encode()]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dens", [0.0, 0.3, 1.0])
def test_string_sources_into_every_integer_target(ctx, dens, where):
    rng = np.random.default_rng(11 + int(dens * 10))
    n = 641
    vals = [None if rng.random() < dens or dens == 1.0 else (NUMBERS[rng.integers(0, len(NUMBERS))] if rng.random() < 0.6 else str(int(rng.integers(-70000, 70000))).encode()) for _ in range(n)]
    col = StrColumn(vals)
    for flags in (abi.CAST_IN_INSERT | abi.CAST_TRUNCATE_AS_WARNING, abi.CAST_IGNORE_TRUNCATE, abi.CAST_TRUNCATE_AS_WARNING):
        want, sc = R.cast_rows(flags, rows_of([col]), [abi.BYTES], INT_TARGETS, [0] * 10)
        got, warn = run_cast(ctx, where, [col], INT_TARGETS, [0] * 10, flags)
        assert got.rows() == [tuple(r) for r in want]
        assert (warn["overflow"], warn["truncated"], warn["bad_null"]) == (sc.warn_overflow, sc.warn_truncated, sc.warn_bad_null)
        if dens == 0.0 and flags & abi.CAST_TRUNCATE_AS_WARNING:
            assert sc.warn_truncated > 100 and sc.warn_overflow > 100 and any(r[1] is None for r in want)  # (the unsigned arm's NULLs)


@pytest.mark.parametrize("where", ["host", "device"])
def test_truncated_wrong_value_and_overflow_of_a_string_are_found_where_they_are(ctx, where):
    n = 700
    base = [b"%d" % (i % 100) for i in range(n)]
    fts = [R.FieldType(abi.TP_TINY), R.FieldType(abi.TP_SHORT, unsigned=True), R.FieldType(abi.TP_VARCHAR, 8, charset="utf8mb4")]
    for row in (0, 63, 64, 127, 128, 511, 512, n - 1):
        for c, bad, code in ((0, b"12abc", abi.ERR_TRUNCATED_WRONG_VALUE), (0, b"128", abi.ERR_OUT_OF_RANGE), (1, b"-1", abi.ERR_OUT_OF_RANGE), (1, b"", abi.ERR_TRUNCATED_WRONG_VALUE),
                             (1, b"99999999999999999999", abi.ERR_OUT_OF_RANGE)):
            v = [list(base), list(base), list(base)]
            v[c][row] = bad
            cols = [StrColumn(x) for x in v]
            with pytest.raises(R.CastError) as w:
                R.cast_rows(abi.CAST_IN_INSERT, rows_of(cols), [abi.BYTES] * 3, fts, [0, 1, 2])
            assert (w.value.row, w.value.col, w.value.code) == (row, c, code)
            with pytest.raises(T.CastError) as e:
                run_cast(ctx, where, cols, fts, [0, 1, 2], abi.CAST_IN_INSERT)
            assert (e.value.row, e.value.column, e.value.status) == (row, c, code)
    # the same statement column feeding an integer and a string column; the string kernel's error in an earlier row wins, and the other way round
    v = [list(base), list(base), list(base)]
    v[0][301], v[2][300] = b"x", b"far too long"
    with pytest.raises(T.CastError) as e:
        run_cast(ctx, where, [StrColumn(x) for x in v], fts, [0, 1, 2], abi.CAST_IN_INSERT)
    assert (e.value.row, e.value.column, e.value.status) == (300, 2, abi.ERR_DATA_TOO_LONG)
    v[0][299] = b"1e9"
    with pytest.raises(T.CastError) as e:
        run_cast(ctx, where, [StrColumn(x) for x in v], fts, [0, 1, 2], abi.CAST_IN_INSERT)
    assert (e.value.row, e.value.column, e.value.status) == (299, 0, abi.ERR_OUT_OF_RANGE)
