"""GPU parity of tsq_rows_equal with types.EqualDatums as tests/dupcheck_ref.py restates it (types/datum.go:896-916,
types/compare.go:104-123): one flag per row pair, compared exactly."""
import numpy as np
import pytest

from tests import dupcheck_gpu_helpers as G
from tests import dupcheck_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import dupcheck as D
from tinysql_amd.chunk import Chunk, Column
from tinysql_amd.gpu_pipeline import DeviceChunk

pytestmark = pytest.mark.gpu

NAN = float("nan")


def run(ctx, types, rows_a, rows_b, idx_a, idx_b, n=None):
    """flags of the pairs (rows_a[idx_a[i]], rows_b[idx_b[i]]); idx None = pair i takes row i"""
    a, b = DeviceChunk.from_host(ctx, R.chunk_of(types, rows_a)), DeviceChunk.from_host(ctx, R.chunk_of(types, rows_b))
    n = n if n is not None else len(idx_a if idx_a is not None else (idx_b if idx_b is not None else rows_a))
    keep = [D.DevArray(ctx, np.array(i, dtype=np.int64)) if i is not None else None for i in (idx_a, idx_b)]
    out = G.Guarded(ctx, n)
    try:
        D.rows_equal(ctx, [c.col(len(rows_a)) for c in a.columns], keep[0].p if keep[0] else None, [c.col(len(rows_b)) for c in b.columns],
                     keep[1].p if keep[1] else None, n, out.p)
        return out.read(np.uint8, n).tolist()
    finally:
        out.free()
        for k in keep:
            if k:
                k.free()
        a.free()
        b.free()


def want(rows_a, rows_b, idx_a, idx_b, n):
    out = []
    for i in range(n):
        ia, ib = (i if idx_a is None else idx_a[i]), (i if idx_b is None else idx_b[i])
        ok = 0 <= ia < len(rows_a) and 0 <= ib < len(rows_b)
        out.append(int(ok and R.equal_datums(rows_a[ia], rows_b[ib])))
    return out


def test_every_pair_of_edge_cells_per_type(ctx):
    cells = {
        abi.I64: [None, 0, 1, -1, -(1 << 63), (1 << 63) - 1],
        abi.U64: [None, 0, 1, (1 << 64) - 1, 1 << 63],
        abi.F64: [None, 0.0, -0.0, 1.5, -1.5, NAN, float("inf"), float("-inf"), 5e-324],
        abi.F32: [None, 0.0, -0.0, 1.5, NAN, float("inf")],
        abi.BYTES: [None, b"", b"\0", b"a", b"abcdefg", b"abcdefh", b"abcdefgh", b"abcdefgi", b"abcdefghi", b"abcdefghj", b"x" * 64, b"x" * 63 + b"y",
                    b"x" * 65, b"x" * 64 + b"y", b"x" * 70],
    }
    for tp, cs in cells.items():
        rows = [(c,) for c in cs]
        ia = [i for i in range(len(cs)) for _ in cs]
        ib = [j for _ in cs for j in range(len(cs))]
        got = run(ctx, [tp], rows, rows, ia, ib)
        assert got == want(rows, rows, ia, ib, len(ia)), tp
    # the pinned points: -0.0 equals 0.0, a NaN equals nothing (itself included), NULL equals NULL and neither 0 nor ""
    assert run(ctx, [abi.F64], [(0.0,), (NAN,), (None,), (None,)], [(-0.0,), (NAN,), (None,), (0.0,)], None, None) == [1, 0, 1, 0]
    assert run(ctx, [abi.BYTES], [(None,), (None,), (b"",)], [(None,), (b"",), (b"",)], None, None) == [1, 0, 1]
    assert run(ctx, [abi.I64], [(None,), (None,), (0,)], [(None,), (0,), (0,)], None, None) == [1, 0, 1]


@pytest.mark.parametrize("n", [0, 1, 63, 64, 65, 1025, 4097])
def test_rows_of_every_type_with_indices(ctx, n):
    rng = np.random.default_rng(n)
    types = [abi.I64, abi.BYTES, abi.F64, abi.U64, abi.F32, abi.BYTES]
    words = [None, b"", b"k", b"key-0001", b"key-0002", b"key-00011", b"a much longer cell that spans several eight-byte pieces....1",
             b"a much longer cell that spans several eight-byte pieces....2"]
    reals = [None, 0.0, -0.0, 2.5, NAN]

    def rows_of(m):
        return [(None if rng.random() < 0.1 else int(rng.integers(0, 3)), words[int(rng.integers(0, len(words)))], reals[int(rng.integers(0, 5))],
                 int(rng.integers(0, 2)), [None, 0.0, 1.0][int(rng.integers(0, 3))], words[int(rng.integers(0, 3))]) for _ in range(m)]
    base = rows_of(12)
    rows_a = [base[int(rng.integers(0, 12))] for _ in range(max(n, 1))]
    rows_b = [base[int(rng.integers(0, 12))] for _ in range(max(n // 2, 1))]
    idx_a = rng.integers(-1, len(rows_a) + 1, n).tolist()  # -1 and one past the end: 0, nothing read
    idx_b = rng.integers(-1, len(rows_b) + 1, n).tolist()
    got = run(ctx, types, rows_a, rows_b, idx_a, idx_b, n)
    w = want(rows_a, rows_b, idx_a, idx_b, n)
    assert got == w
    assert n < 63 or 0 < sum(w) < n
    # identity on one side, as the executor calls it against the statement's own rows
    idx = rng.integers(-1, len(rows_a), n).tolist()
    assert run(ctx, types, rows_a, rows_a, None, idx, n) == want(rows_a, rows_a, None, idx, n)


def test_no_columns_and_refusals(ctx):
    out = G.Guarded(ctx, 4)
    a = DeviceChunk.from_host(ctx, Chunk([Column(abi.I64, [1, 2, 3])]))
    b = DeviceChunk.from_host(ctx, Chunk([Column(abi.F64, [1.0, 2.0, 3.0])]))
    try:
        D.rows_equal(ctx, [], None, [], None, 4, out.p)  # rows without columns are equal
        assert out.read(np.uint8, 4).tolist() == [1, 1, 1, 1]
        with pytest.raises(_lib.TsqError, match="column types differ") as e:
            D.rows_equal(ctx, [a.columns[0].col(3)], None, [b.columns[0].col(3)], None, 3, out.p)
        assert e.value.status == abi.ERR_INVALID
        host = a.columns[0].col(3)
        host.flags = 0
        with pytest.raises(_lib.TsqError, match="device resident"):
            D.rows_equal(ctx, [host], None, [a.columns[0].col(3)], None, 3, out.p)
        with pytest.raises(_lib.TsqError, match="lengths differ"):
            D.rows_equal(ctx, [a.columns[0].col(3), a.columns[0].col(2)], None, [a.columns[0].col(3), a.columns[0].col(3)], None, 2, out.p)
    finally:
        out.free()
        a.free()
        b.free()
