"""GPU: tsq_cast_run through the C-ABI, bit for bit against tests/cast_ref.py (pinned on the reference's vectors by
tests/test_cast_cpu.py), for host chunks and device chunks: the row counts at which the kernel changes its path, every (source,
target) pair the library takes at three NULL densities, the position and kind of the first error, the same inputs as warnings and
with truncation ignored, defaults, the NOT NULL rule, and every combination tsq_cast_create refuses."""
import ctypes as C
import math

import numpy as np
import pytest

from tests import cast_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import table as T
from tinysql_amd.chunk import Chunk, Column, np_dtype
from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceColumn

pytestmark = pytest.mark.gpu

INT_TPS = (abi.TP_TINY, abi.TP_SHORT, abi.TP_INT24, abi.TP_LONG, abi.TP_LONGLONG)
# the kernel's edges: a wave step of the two-rows-per-lane part is 128 rows, a workgroup's 512; the rest goes 64 rows per wave
ROW_COUNTS = [0, 1, 63, 64, 65, 127, 128, 129, 511, 512, 513, 1025]


def info(ft):
    flag = (T.UnsignedFlag if ft.unsigned else 0) | (T.NotNullFlag if ft.not_null else 0) | (T.AutoIncrementFlag if ft.auto_increment else 0)
    return T.ColumnInfo(ft.tp, ft.flen, ft.decimal, flag, DefaultValue=ft.default)


def stmt_of(flags):
    return T.StatementContext(IgnoreTruncate=bool(flags & abi.CAST_IGNORE_TRUNCATE), TruncateAsWarning=bool(flags & abi.CAST_TRUNCATE_AS_WARNING),
                              OverflowAsWarning=bool(flags & abi.CAST_OVERFLOW_AS_WARNING), BadNullAsWarning=bool(flags & abi.CAST_BAD_NULL_AS_WARNING),
                              InInsertStmt=bool(flags & abi.CAST_IN_INSERT))


def column_of(tp, vals):
    nn = np.array([v is not None for v in vals], dtype=bool)
    return Column(tp, np.array([0 if v is None else v for v in vals], dtype=np_dtype(tp)), nn)


def in_rows(cols):
    """the select's rows as cast_ref takes them (a float32 cell widened)"""
    vals = [[None if c.IsNull(i) else (float(c.data[i]) if c.tp in (abi.F32, abi.F64) else int(c.data[i])) for i in range(len(c))] for c in cols]
    return [list(r) for r in zip(*vals)] if vals and len(vals[0]) else []


def bits_of(tp, v):
    return np.array([v], dtype=np_dtype(tp)).view(np.uint32 if tp == abi.F32 else np.uint64)[0]


def assert_same(got_chunk, want_rows, fts):
    assert got_chunk.NumRows() == len(want_rows)
    for c, ft in enumerate(fts):
        col = got_chunk.columns[c]
        assert col.tp == ft.out_type()
        want = [r[c] for r in want_rows]
        gnull = [col.IsNull(i) for i in range(len(want))]
        assert gnull == [w is None for w in want], "NULLs of column %d differ" % c
        live = [i for i, w in enumerate(want) if w is not None]
        w = np.array([want[i] for i in live], dtype=np_dtype(col.tp))
        g = col.data[live]
        view = np.uint32 if col.tp == abi.F32 else np.uint64
        neq = g.view(view) != w.view(view)
        if col.tp in (abi.F32, abi.F64):
            neq &= ~(np.isnan(w) & np.isnan(g))  # (a NaN passes through a float column without (M, D): any NaN is "the" NaN)
        bad = np.nonzero(neq)[0]
        assert bad.size == 0, "column %d row %d: got %r want %r" % (c, live[bad[0]], g[bad[0]], w[bad[0]])


def run_cast(ctx, where, cols, fts, src_cols, flags):
    """-> (host chunk of the table's columns, warnings); raises table.CastError"""
    types = [c.tp for c in cols]
    caster = T.Caster(ctx, [info(f) for f in fts], src_cols, types, stmt_of(flags))
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


def source_values(rng, tp, n):
    """values around every integer type's bounds, small ones, halves; NaN left out (it fails a run into an integer column)"""
    edges = [0, 1, -1, 127, 128, -128, -129, 255, 256, 32767, 32768, -32769, 65535, 65536, (1 << 23) - 1, 1 << 23, -(1 << 23) - 1, (1 << 24) - 1, 1 << 24,
             (1 << 31) - 1, 1 << 31, -(1 << 31) - 1, (1 << 32) - 1, 1 << 32, (1 << 63) - 1, -(1 << 63), (1 << 64) - 1, 1 << 63]
    out = []
    for _ in range(n):
        k = rng.integers(0, 4)
        e = edges[rng.integers(0, len(edges))]
        if tp in (abi.I64, abi.U64):
            v = e + int(rng.integers(-2, 3)) if k < 2 else int(rng.integers(-300, 300)) if k == 2 else int(rng.integers(-(1 << 62), 1 << 62))
            lo, hi = (R.I64MIN, R.I64MAX) if tp == abi.I64 else (0, R.U64MAX)
            out.append(min(max(v, lo), hi))
        else:
            v = float(e) + float(rng.choice([-1.0, -0.5, -0.25, 0.0, 0.25, 0.5, 1.0])) if k < 2 else round(float(rng.uniform(-1200, 1200)), int(rng.integers(0, 4))) \
                if k == 2 else float(rng.choice([math.inf, -math.inf, 1e300, -1e300, 999.995, 99999999.5, 1e10, -0.0, 0.49999999999999994]))
            out.append(R.to_f32(v) if tp == abi.F32 else v)
    return out


ALL_TARGETS = [R.FieldType(tp, unsigned=u) for tp in INT_TPS for u in (False, True)] + [
    R.FieldType(abi.TP_FLOAT), R.FieldType(abi.TP_DOUBLE), R.FieldType(abi.TP_FLOAT, 5, 2), R.FieldType(abi.TP_DOUBLE, 10, 0), R.FieldType(abi.TP_DOUBLE, 8, 2, unsigned=True),
    R.FieldType(abi.TP_DOUBLE, 40, 8)]


@pytest.fixture(scope="module")
def pair_cases():
    """per (source type, NULL density): the source column and cast_ref's rows for all sixteen targets, computed once"""
    out = {}
    n = 641  # five wave steps of the two-row part + one row
    for st in (abi.I64, abi.U64, abi.F32, abi.F64):
        for dens in (0.0, 0.3, 1.0):
            rng = np.random.default_rng(100 * st + int(dens * 10))
            vals = source_values(rng, st, n)
            nulls = rng.random(n) < dens if dens < 1.0 else np.ones(n, bool)
            col = column_of(st, [None if nulls[i] else v for i, v in enumerate(vals)])
            flags = abi.CAST_IN_INSERT | abi.CAST_TRUNCATE_AS_WARNING
            rows, sc = R.cast_rows(flags, in_rows([col]), [st], ALL_TARGETS, [0] * len(ALL_TARGETS))
            out[(st, dens)] = (col, flags, rows, sc)
    return out


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("dens", [0.0, 0.3, 1.0])
@pytest.mark.parametrize("st", [abi.I64, abi.U64, abi.F32, abi.F64], ids=["i64", "u64", "f32", "f64"])
def test_every_pair_at_three_null_densities(ctx, pair_cases, st, dens, where):
    col, flags, rows, sc = pair_cases[(st, dens)]
    got, warn = run_cast(ctx, where, [col], ALL_TARGETS, [0] * len(ALL_TARGETS), flags)
    assert_same(got, rows, ALL_TARGETS)
    assert (warn["overflow"], warn["bad_null"]) == (sc.warn_overflow, sc.warn_bad_null)
    if dens == 0.0:
        assert sc.warn_overflow > 0  # (the inputs do leave the ranges)


# table (id BIGINT AUTO_INCREMENT, a INT, b TINYINT UNSIGNED NOT NULL, c DOUBLE(8,2), d FLOAT, e SMALLINT DEFAULT 7, f INT DEFAULT NULL) fed by
# (BIGINT a, BIGINT b, DOUBLE c, DOUBLE d) — the statement names (c, a, b, d): e, f and id take their defaults
MIX_FTS = [R.FieldType(abi.TP_LONGLONG, not_null=True, auto_increment=True), R.FieldType(abi.TP_LONG), R.FieldType(abi.TP_TINY, unsigned=True, not_null=True),
           R.FieldType(abi.TP_DOUBLE, 8, 2), R.FieldType(abi.TP_FLOAT), R.FieldType(abi.TP_SHORT, default=7), R.FieldType(abi.TP_LONG)]
MIX_SRC = [-1, 1, 2, 0, 3, -1, -1]
MIX_TYPES = [abi.F64, abi.I64, abi.I64, abi.F64]


def mix_chunk(n, seed=5, null_a=True):
    rng = np.random.default_rng(seed)
    c = Column(abi.F64, np.round(rng.uniform(-99999, 99999, n), 3), rng.random(n) > 0.2)
    a = Column(abi.I64, rng.integers(-(1 << 31), 1 << 31, n), rng.random(n) > 0.3 if null_a else None)
    b = Column(abi.I64, rng.integers(0, 256, n))
    d = Column(abi.F64, rng.uniform(-1e6, 1e6, n), rng.random(n) > 0.1)
    return [c, a, b, d]


@pytest.fixture(scope="module")
def mix_ref():
    cols = mix_chunk(1025 * 1)
    rows, sc = R.cast_rows(abi.CAST_IN_INSERT, in_rows(cols), MIX_TYPES, MIX_FTS, MIX_SRC)
    return cols, rows


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", ROW_COUNTS)
def test_row_counts_at_the_kernels_edges(ctx, mix_ref, n, where):
    cols, rows = mix_ref
    got, warn = run_cast(ctx, where, [c.slice(0, n) for c in cols], MIX_FTS, MIX_SRC, abi.CAST_IN_INSERT)
    assert_same(got, rows[:n], MIX_FTS)
    assert warn == {"overflow": 0, "truncated": 0, "data_too_long": 0, "bad_null": 0, "bad_utf8": 0}


def test_more_rows_than_one_pass_of_the_grid(ctx):
    """the grid is capped at eight workgroups per CU: beyond 8 * CUs * 512 rows a workgroup takes a second step.  The input repeats a
    1000-row pattern (no multiple of a wave step), so cast_ref is computed on 1000 rows"""
    period, n = 1000, 8 * 256 * 512 * 2 + 513
    cols = mix_chunk(period, seed=9)
    rows, _ = R.cast_rows(abi.CAST_IN_INSERT, in_rows(cols), MIX_TYPES, MIX_FTS, MIX_SRC)
    reps = n // period + 1
    big = [Column(c.tp, np.tile(c.data, reps)[:n], None if c.notnull is None else np.tile(c.notnull, reps)[:n]) for c in cols]
    got, _ = run_cast(ctx, "device", big, MIX_FTS, MIX_SRC, abi.CAST_IN_INSERT)
    want = Chunk([column_of(ft.out_type(), [r[c] for r in rows]) for c, ft in enumerate(MIX_FTS)])
    for c, ft in enumerate(MIX_FTS):
        g, w = got.columns[c], want.columns[c]
        wn = np.ones(period, bool) if w.notnull is None else w.notnull
        gn = np.ones(n, bool) if g.notnull is None else g.notnull
        assert (gn == np.tile(wn, reps)[:n]).all(), c
        view = np.uint32 if g.tp == abi.F32 else np.uint64
        assert (g.data.view(view) == np.tile(w.data, reps)[:n].view(view)).all(), c


def test_buffers_that_are_not_16_byte_aligned_take_the_row_per_lane_path(ctx):
    cols, n = mix_chunk(700, seed=11), 700
    rows, _ = R.cast_rows(abi.CAST_IN_INSERT, in_rows(cols), MIX_TYPES, MIX_FTS, MIX_SRC)
    caster = T.Caster(ctx, [info(f) for f in MIX_FTS], MIX_SRC, MIX_TYPES, stmt_of(abi.CAST_IN_INSERT))
    dchk = DeviceChunk.from_host(ctx, Chunk(cols))
    out = [DeviceColumn(ctx, ft.out_type(), n + 8) for ft in MIX_FTS]
    try:
        shifted = [DeviceColumn(ctx, c.tp, n, data=c.data + 8, bitmap=c.bitmap + 1) for c in out]  # 8 bytes into the data, 1 into the bitmap
        oc = (abi.Col * len(out))(*[c.col(n) for c in shifted])
        _lib.check(ctx.lib.tsq_cast_run(caster.h, dchk.cols(), 4, n, oc, None, None), caster.h)
        assert_same(DeviceChunk(shifted, n).to_host(), rows, MIX_FTS)
    finally:
        for c in out:
            c.free()
        dchk.free()
        caster.close()


# ---------------------------------------------------------------- errors
ERR_FTS = [R.FieldType(abi.TP_TINY), R.FieldType(abi.TP_SHORT, unsigned=True), R.FieldType(abi.TP_LONG, not_null=True)]
ERR_N = 1025


def err_cols(bad):
    """three BIGINT columns of in-range values; bad: [(row, statement column, value or None)]"""
    vals = [[(r * 7 + c) % 100 for r in range(ERR_N)] for c in range(3)]
    for r, c, v in bad:
        vals[c][r] = v
    return [column_of(abi.I64, v) for v in vals]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("row", [0, ERR_N - 1, 63, 64, 127, 128, 511, 512, 1023, 1024])
def test_a_single_bad_cell_is_found_where_it_is(ctx, row, where):
    for c, v, code in ((0, 128, abi.ERR_OUT_OF_RANGE), (1, -1, abi.ERR_OUT_OF_RANGE), (2, None, abi.ERR_BAD_NULL)):
        with pytest.raises(T.CastError) as e:
            run_cast(ctx, where, err_cols([(row, c, v)]), ERR_FTS, [0, 1, 2], abi.CAST_IN_INSERT)
        assert (e.value.row, e.value.column, e.value.status) == (row, c, code)


@pytest.mark.parametrize("where", ["host", "device"])
def test_the_first_error_in_row_then_statement_column_order_wins(ctx, where):
    # statement (c2, c1, c0): src_cols maps table column -> statement column
    src = [2, 1, 0]
    cases = [
        [(700, 0, 999), (300, 1, -5)],            # different rows: the earlier row
        [(300, 0, 1 << 40), (300, 1, 70000)],     # one row: statement column 0 (it feeds table column 2) comes first
        [(64, 2, 999), (64, 1, -5), (63, 0, None)],  # row 63's NOT NULL failure (table column 2) is before row 64's casts
        [(500, 0, None), (500, 2, 999)],          # one row: the cast error of statement column 2 comes before the NOT NULL pass
    ]
    for bad in cases:
        cols = err_cols(bad)
        try:
            R.cast_rows(abi.CAST_IN_INSERT, in_rows(cols), [abi.I64] * 3, ERR_FTS, src)
            raise AssertionError("the reference finds no error in %r" % (bad,))
        except R.CastError as w:
            with pytest.raises(T.CastError) as e:
                run_cast(ctx, where, cols, ERR_FTS, src, abi.CAST_IN_INSERT)
            assert (e.value.row, e.value.column, e.value.status) == (w.row, w.col, w.code), bad
    # the two bad cells of one row in statement order, spelled out: statement column 0 feeds table column 2, column 1 table column 1
    cols = err_cols([(300, 0, 1 << 40), (300, 1, 70000)])
    with pytest.raises(T.CastError) as e:
        run_cast(ctx, where, cols, ERR_FTS, src, abi.CAST_IN_INSERT)
    assert (e.value.row, e.value.column) == (300, 2)


@pytest.mark.parametrize("where", ["host", "device"])
def test_the_same_bad_cells_as_warnings_and_ignored(ctx, where):
    bad = [(0, 0, 128), (63, 1, -1), (64, 0, -129), (511, 1, 65536), (512, 2, 1 << 40), (1024, 0, 999), (700, 2, None)]
    cols = err_cols(bad)
    for flags in (abi.CAST_IN_INSERT | abi.CAST_TRUNCATE_AS_WARNING | abi.CAST_BAD_NULL_AS_WARNING,
                  abi.CAST_IN_INSERT | abi.CAST_IGNORE_TRUNCATE | abi.CAST_BAD_NULL_AS_WARNING, abi.CAST_TRUNCATE_AS_WARNING | abi.CAST_BAD_NULL_AS_WARNING):
        rows, sc = R.cast_rows(flags, in_rows(cols), [abi.I64] * 3, ERR_FTS, [0, 1, 2])
        got, warn = run_cast(ctx, where, cols, ERR_FTS, [0, 1, 2], flags)
        assert_same(got, rows, ERR_FTS)
        assert (warn["overflow"], warn["bad_null"]) == (sc.warn_overflow, sc.warn_bad_null)
        assert warn["bad_null"] == 1 and warn["overflow"] == (0 if flags & abi.CAST_IGNORE_TRUNCATE else 6)
        assert rows[0][0] == 127 and rows[700][2] == 0 and rows[63][1] == (0 if flags & abi.CAST_IN_INSERT else 65535)
    # without BAD_NULL_AS_WARNING the NULL is the statement's error although truncation is ignored
    with pytest.raises(T.CastError) as e:
        run_cast(ctx, where, cols, ERR_FTS, [0, 1, 2], abi.CAST_IN_INSERT | abi.CAST_IGNORE_TRUNCATE)
    assert (e.value.row, e.value.column, e.value.status) == (700, 2, abi.ERR_BAD_NULL)


def test_float_overflow_as_warning_and_the_unsigned_rule(ctx):
    fts = [R.FieldType(abi.TP_DOUBLE, 5, 2), R.FieldType(abi.TP_DOUBLE, 5, 2, unsigned=True), R.FieldType(abi.TP_FLOAT, unsigned=True)]
    col = column_of(abi.F64, [1.005, 999.994, 999.995, -999.995, 1e9, -1e9, float("nan"), -0.001, 0.0] * 20)
    for flags in (abi.CAST_OVERFLOW_AS_WARNING | abi.CAST_TRUNCATE_AS_WARNING, abi.CAST_TRUNCATE_AS_WARNING, abi.CAST_OVERFLOW_AS_WARNING | abi.CAST_IGNORE_TRUNCATE):
        rows, sc = R.cast_rows(flags, in_rows([col]), [abi.F64], fts, [0, 0, 0])
        got, warn = run_cast(ctx, "device", [col], fts, [0, 0, 0], flags)
        assert_same(got, rows, fts)
        assert warn["overflow"] == sc.warn_overflow and sc.warn_overflow > 0
    with pytest.raises(R.CastError) as w:  # strict: the first value beyond DOUBLE(5,2)
        R.cast_rows(0, in_rows([col]), [abi.F64], fts, [0, 0, 0])
    with pytest.raises(T.CastError) as e:
        run_cast(ctx, "device", [col], fts, [0, 0, 0], 0)
    assert (e.value.row, e.value.column, e.value.status) == (w.value.row, w.value.col, abi.ERR_OUT_OF_RANGE) and w.value.row < 9


def test_a_nan_for_an_integer_column_is_unsupported_whatever_the_flags(ctx):
    col = column_of(abi.F64, [1.5] * 200 + [float("nan")] + [2.5] * 50)
    for flags in (0, abi.CAST_IGNORE_TRUNCATE, abi.CAST_TRUNCATE_AS_WARNING | abi.CAST_IN_INSERT):
        for ft in (R.FieldType(abi.TP_LONG), R.FieldType(abi.TP_LONGLONG, unsigned=True)):
            with pytest.raises(T.CastError) as e:
                run_cast(ctx, "device", [col], [ft], [0], flags)
            assert (e.value.row, e.value.column, e.value.status) == (200, 0, abi.ERR_UNSUPPORTED)
    got, _ = run_cast(ctx, "device", [col], [R.FieldType(abi.TP_DOUBLE)], [0], 0)  # ... and passes through a DOUBLE column
    assert math.isnan(got.columns[0].data[200])


def test_defaults_are_cast_once_by_the_host_layer(ctx):
    fts = [R.FieldType(abi.TP_LONG), R.FieldType(abi.TP_TINY, default=127), R.FieldType(abi.TP_DOUBLE, 6, 1, default=2.3), R.FieldType(abi.TP_FLOAT, default=R.to_f32(0.1)),
           R.FieldType(abi.TP_LONGLONG, unsigned=True, not_null=True, default=(1 << 64) - 1), R.FieldType(abi.TP_LONG)]
    infos = [info(f) for f in fts]
    infos[1].DefaultValue, infos[2].DefaultValue, infos[3].DefaultValue = 300, 2.25, 0.1  # as the DDL keeps them: cast when the handle is made
    col = column_of(abi.I64, list(range(130)))
    caster = T.Caster(ctx, infos, [0, -1, -1, -1, -1, -1], [abi.I64], T.StatementContext(TruncateAsWarning=True))
    try:
        got = caster.run(Chunk([col]))
    finally:
        caster.close()
    rows, _ = R.cast_rows(abi.CAST_IN_INSERT, in_rows([col]), [abi.I64], fts, [0, -1, -1, -1, -1, -1])
    assert_same(got, rows, fts)
    assert got.rows()[5] == (5, 127, 2.3, float(np.float32(0.1)), (1 << 64) - 1, None)


# ---------------------------------------------------------------- create-time and argument checks
def create(ctx, specs, stmt_flags=0):
    arr = (abi.CastCol * len(specs))()
    for s, (src_col, src_type, tp, flags) in zip(arr, specs):
        s.src_col, s.src_type, s.tp, s.flen, s.decimal, s.flags = src_col, src_type, tp, -1, -1, flags
    h = C.c_void_p()
    st = ctx.lib.tsq_cast_create(ctx.h, arr, len(specs), stmt_flags, 0, C.byref(h))
    if st == abi.OK:
        ctx.lib.tsq_cast_destroy(h)
    return st


def test_create_refuses_what_the_go_path_keeps(ctx):
    strings = (abi.TP_VARCHAR, abi.TP_VAR_STRING, abi.TP_STRING, abi.TP_BLOB, abi.TP_TINY_BLOB, abi.TP_MEDIUM_BLOB, abi.TP_LONG_BLOB)
    listed = [(0, abi.F32, tp, 0) for tp in strings] + [(0, abi.F64, tp, 0) for tp in strings]          # a float source into a string target
    listed += [(0, abi.BYTES, abi.TP_FLOAT, 0), (0, abi.BYTES, abi.TP_DOUBLE, 0)]                          # a string source into FLOAT / DOUBLE
    listed += [(0, t, abi.TP_BIT, 0) for t in (abi.I64, abi.U64, abi.F64, abi.BYTES)]                      # TypeBit targets
    listed += [(0, abi.I64, abi.TP_LONGLONG, abi.CAST_AUTO_INCREMENT | abi.CAST_UNSIGNED), (0, abi.F64, abi.TP_DOUBLE, abi.CAST_AUTO_INCREMENT),
               (0, abi.F64, abi.TP_FLOAT, abi.CAST_AUTO_INCREMENT)]                                        # an unsigned / floating auto-increment column
    for spec in listed:
        assert create(ctx, [spec]) == abi.ERR_UNSUPPORTED, spec
        assert create(ctx, [(0, abi.I64, abi.TP_LONG, 0), spec]) == abi.ERR_UNSUPPORTED, spec
    assert create(ctx, [(0, abi.I64, abi.TP_LONG, 0)] * 17) == abi.ERR_UNSUPPORTED  # more than TSQ_MAX_COLS columns
    # every pair the library does take
    for t in (abi.I64, abi.U64, abi.F32, abi.F64):
        for tp in INT_TPS + (abi.TP_FLOAT, abi.TP_DOUBLE):
            for f in (0, abi.CAST_UNSIGNED):
                assert create(ctx, [(0, t, tp, f)]) == abi.OK
    for tp in INT_TPS:
        for f in (0, abi.CAST_UNSIGNED):
            assert create(ctx, [(0, abi.BYTES, tp, f)]) == abi.OK
    for t in (abi.I64, abi.U64, abi.BYTES):
        for tp in strings:
            for f in (0, abi.CAST_CHARSET_BIN, abi.CAST_CHARSET_UTF8, abi.CAST_CHARSET_UTF8MB4):
                assert create(ctx, [(0, t, tp, f)]) == abi.OK
    assert create(ctx, [(0, abi.I64, 6, 0)]) == abi.ERR_INVALID and create(ctx, [(0, abi.I64, abi.TP_LONG, 0)], stmt_flags=64) == abi.ERR_INVALID
    assert create(ctx, [(0, 9, abi.TP_LONG, 0)]) == abi.ERR_INVALID and create(ctx, [(-2, abi.I64, abi.TP_LONG, 0)]) == abi.ERR_INVALID


def test_run_checks_its_arguments_and_cancel_sticks(ctx):
    caster = T.Caster(ctx, [T.ColumnInfo(abi.TP_LONG)], [0], [abi.I64], T.StatementContext())
    try:
        lib, keep = ctx.lib, []
        from tinysql_amd.chunk import make_cols, out_buffers
        ins = make_cols([Column(abi.I64, np.arange(10))], keep)
        outs, _ = out_buffers([abi.I64], 10, keep)
        wrong, _ = out_buffers([abi.U64], 10, keep)
        assert lib.tsq_cast_run(caster.h, ins, 1, 10, wrong, None, None) == abi.ERR_INVALID       # the output column's type
        assert lib.tsq_cast_run(caster.h, ins, 0, 10, outs, None, None) == abi.ERR_INVALID        # src_col beyond the inputs
        assert lib.tsq_cast_run(caster.h, ins, 1, 11, outs, None, None) == abi.ERR_INVALID        # more rows than the input holds
        assert lib.tsq_cast_run(caster.h, make_cols([Column(abi.F64, np.zeros(10))], keep), 1, 10, outs, None, None) == abi.ERR_INVALID
        assert lib.tsq_cast_run(caster.h, ins, 1, 1 << 31, outs, None, None) == abi.ERR_UNSUPPORTED
        row, col = C.c_int64(0), C.c_int32(0)
        assert lib.tsq_cast_run(caster.h, ins, 1, 10, outs, None, None) == abi.OK
        assert lib.tsq_cast_error_at(caster.h, C.byref(row), C.byref(col)) == abi.ERR_INVALID      # the last run had no error
        assert caster.stats()["rows"] == 10 and caster.stats()["launches"] == 1
        assert lib.tsq_cast_cancel(caster.h) == abi.OK
        assert lib.tsq_cast_run(caster.h, ins, 1, 10, outs, None, None) == abi.ERR_CANCELLED
    finally:
        caster.close()
