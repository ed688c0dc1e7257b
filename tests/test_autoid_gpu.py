"""GPU: tsq_autoid_fill — the auto-increment ids of a chunk as a three-launch scan — against the sequential loop of
tests/cast_ref.py (adjustAutoIncrementDatum, executor/insert_common.go:594-638; pinned on the reference's sequences by
tests/test_cast_cpu.py).  Sizes around the 1024-row tile and one at which the second-level scan holds more tiles than a wave has
lanes; the patterns that move the allocator in every way."""
import numpy as np
import pytest

from tests import cast_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import table as T
from tinysql_amd.chunk import Column
from tinysql_amd.gpu_pipeline import DeviceColumn

pytestmark = pytest.mark.gpu

TILE = 1024
SIZES = [0, 1, 64, 65, TILE - 1, TILE, TILE + 1, TILE * 256 + 3]
INT = T.ColumnInfo(abi.TP_LONG, Flag=T.AutoIncrementFlag | T.NotNullFlag)
BIG = T.ColumnInfo(abi.TP_LONGLONG, Flag=T.AutoIncrementFlag | T.NotNullFlag)


def pattern(name, n):
    """-> list of None / int"""
    rng = np.random.default_rng(n + len(name))
    if name == "all_null":
        return [None] * n
    if name == "explicit_ascending":
        return [10 + 3 * i for i in range(n)]
    if name == "explicit_descending":
        return [10 + 3 * (n - i) for i in range(n)]
    if name == "explicit_equal":
        return [77] * n
    if name == "explicit_at_tile_boundaries":  # an explicit id on the last row of a tile and on the first row of the next, NULLs between
        v = [None] * n
        for t in range(TILE, n + 1, TILE):
            v[t - 1] = 5 * t
            if t < n:
                v[t] = 5 * t - 7 if (t // TILE) % 2 else 5 * t + 100
        return v
    if name == "zeros":
        return [0 if rng.random() < 0.4 else None if rng.random() < 0.5 else int(rng.integers(1, 3 * n + 2)) for _ in range(n)]
    if name == "negative_explicit":
        return [int(-rng.integers(1, 1 << 40)) if rng.random() < 0.3 else None if rng.random() < 0.6 else int(rng.integers(1, 50)) for _ in range(n)]
    if name == "mixed":
        return [None if rng.random() < 0.7 else int(rng.integers(1, 2 * n + 10)) for _ in range(n)]
    raise KeyError(name)


def run(ctx, where, vals, base, info, no_zero=False):
    n = len(vals)
    col = Column(abi.I64, np.array([0 if v is None else v for v in vals], dtype=np.int64), np.array([v is not None for v in vals], dtype=bool))
    stmt = T.StatementContext(NoAutoValueOnZero=no_zero)
    if where == "host":
        out, nb, first, last = T.FillAutoID(ctx, col, n, base, info, stmt)
        assert out.notnull is None
        return out.data.tolist(), nb, first, last
    d = DeviceColumn(ctx, abi.I64, n)
    try:
        if n:
            ctx.h2d(d.data, col.data)
            ctx.h2d(d.bitmap, np.packbits(col.notnull if col.notnull is not None else np.ones(n, bool), bitorder="little"))
        _, nb, first, last = T.FillAutoID(ctx, d, n, base, info, stmt)
        h = d.to_host(n)
        assert h.notnull is None  # every row is NOT NULL afterwards (and no bit behind the last row is set: Column would keep them apart)
        bm = np.zeros((n + 7) // 8 + 1, np.uint8)
        if n:
            ctx.d2h(bm, d.bitmap)
            assert (np.unpackbits(bm[:(n + 7) // 8], bitorder="little")[n:] == 0).all()
        return h.data.tolist(), nb, first, last
    finally:
        d.free()


@pytest.fixture(scope="module")
def refs():
    cache = {}

    def get(name, n, base, no_zero=False, upper=R.I64MAX):
        key = (name, n, base, no_zero, upper)
        if key not in cache:
            vals = pattern(name, n)
            cache[key] = (vals, R.fill_auto_ids(vals, base, no_zero, upper))
        return cache[key]
    return get


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("n", SIZES)
@pytest.mark.parametrize("name", ["all_null", "explicit_ascending", "explicit_descending", "explicit_equal", "explicit_at_tile_boundaries", "negative_explicit", "mixed"])
def test_patterns_equal_the_sequential_loop(ctx, refs, name, n, where):
    base = 41
    vals, want = refs(name, n, base)
    assert run(ctx, where, vals, base, BIG) == want


@pytest.mark.parametrize("no_zero", [False, True])
@pytest.mark.parametrize("n", [65, TILE + 1, TILE * 256 + 3])
def test_zeros_with_and_without_no_auto_value_on_zero(ctx, refs, n, no_zero):
    vals, want = refs("zeros", n, 0, no_zero)
    got = run(ctx, "device", vals, 0, BIG, no_zero)
    assert got == want
    if no_zero:
        assert 0 in got[0]


@pytest.mark.parametrize("where", ["host", "device"])
@pytest.mark.parametrize("bad_row", [0, 63, 64, TILE - 1, TILE, 3 * TILE + 17, TILE * 256 + 2])
def test_the_bound_error_names_its_row(ctx, bad_row, where):
    """an INT column (upper bound 2^31 - 1): NULLs up to the chosen row, where the allocator leaves the type's range; rows after it
    would fail too — the first one is the statement's error"""
    n = TILE * 256 + 3
    upper = (1 << 31) - 1
    base = upper - bad_row
    vals = [None] * n
    with pytest.raises(R.AutoIdError) as w:
        R.fill_auto_ids(vals, base, False, upper)
    assert (w.value.row, w.value.code) == (bad_row, abi.ERR_OUT_OF_RANGE)
    with pytest.raises(T.AutoIDError) as e:
        run(ctx, where, vals, base, INT)
    assert (e.value.row, e.value.status) == (bad_row, abi.ERR_OUT_OF_RANGE)
    # an explicit id AT the bound is fine, the next allocation is not
    vals = [None, upper, 5, None]
    with pytest.raises(T.AutoIDError) as e:
        run(ctx, where, vals, 7, INT)
    assert (e.value.row, e.value.status) == (3, abi.ERR_OUT_OF_RANGE)
    assert run(ctx, where, vals[:3], 7, INT) == ([8, upper, 5], upper, 8, 5)


def test_passing_int64_max_is_unsupported_and_arguments_are_checked(ctx):
    import ctypes as C
    top = R.I64MAX
    assert run(ctx, "device", [None, top - 1, None], 3, BIG) == ([4, top - 1, top], top, 4, top - 1)
    with pytest.raises(T.AutoIDError) as e:
        run(ctx, "device", [None, top - 1, None, 9, None] + [None] * 2000, 3, BIG)
    assert e.value.status == abi.ERR_UNSUPPORTED
    with pytest.raises(T.AutoIDError) as e:
        run(ctx, "device", [None] * 5, top - 2, BIG)
    assert e.value.status == abi.ERR_UNSUPPORTED
    with pytest.raises(T.AutoIDError) as e:  # a negative base: an allocator never has one
        run(ctx, "host", [None], -1, BIG)
    assert e.value.status == abi.ERR_INVALID
    col = abi.Col()
    col.type, col.length = abi.U64, 0
    nb = C.c_int64(0)
    assert ctx.lib.tsq_autoid_fill(ctx.h, C.byref(col), 0, 0, 0, 127, C.byref(nb), None, None, None) == abi.ERR_UNSUPPORTED  # an unsigned id column
    col.type = abi.I64
    assert ctx.lib.tsq_autoid_fill(ctx.h, C.byref(col), 0, 0, 2, 127, C.byref(nb), None, None, None) == abi.ERR_INVALID      # an unknown flag
    assert ctx.lib.tsq_autoid_fill(ctx.h, C.byref(col), 0, 5, 0, 127, C.byref(nb), None, None, None) == abi.OK and nb.value == 5


def test_a_column_without_a_bitmap_has_no_nulls(ctx):
    vals = [0, 5, 0, 0, 3, 0] * 300
    want = R.fill_auto_ids(vals, 2)
    d = DeviceColumn(ctx, abi.I64, len(vals), with_bitmap=False)
    try:
        ctx.h2d(d.data, np.array(vals, dtype=np.int64))
        _, nb, first, last = T.FillAutoID(ctx, d, len(vals), 2, BIG, T.StatementContext())
        assert (d.to_host(len(vals)).data.tolist(), nb, first, last) == want
    finally:
        d.free()
