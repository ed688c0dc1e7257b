"""GPU parity of tsq_rowcodec_encode (chunk rows -> stored rows in row format v2: what tables.AddRecord writes through
rowcodec.Encoder.Encode, util/rowcodec/encoder.go:34-194) against the oracle's restatement of the encoder: byte-identical rows and row
boundaries at tile-boundary sizes, every schema shape (small / large by id / 16 columns / every fixed-width type at its width edges),
NULL patterns, string columns through the staged and the direct path in one launch, the 65534 / 65535 / 65536-byte rows, bit columns,
host and device placement at every alignment of the output pointer, the round trip through tsq_rowcodec_decode, and the contracts."""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import rowcodec as RC
from tinysql_amd.chunk import Chunk, Column, StrColumn, make_cols
from tinysql_amd.gpu_pipeline import DeviceChunk

pytestmark = pytest.mark.gpu

SIGNED = [0, 1, -1, 127, 128, -128, -129, 32767, 32768, -32768, -32769, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, -(1 << 31), -(1 << 31) - 1, -(1 << 31) + 1,
          (1 << 63) - 1, -(1 << 63)]
UNSIGNED = [0, 1, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
F64S = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1.5, -2.25, 1e300]
F32S = [0.1, -0.1, 1.5, float("inf"), 16777217.0]


def fixed_chunk(rng, n, null_p=0.2, nan=True):
    iv = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64) >> rng.integers(0, 64, n)
    uv = (rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64)).astype(np.uint64)
    fv = np.ldexp(rng.random(n) - 0.5, rng.integers(-60, 60, n))
    f32 = (rng.random(n) * 100 - 50).astype(np.float32)
    k = min(n, len(SIGNED))
    iv[:k] = np.array(SIGNED[:k], dtype=np.int64)
    k = min(n, len(UNSIGNED))
    uv[:k] = np.array(UNSIGNED[:k], dtype=np.uint64)
    vals = F64S if nan else [v for v in F64S if v == v]
    k = min(n, len(vals))
    fv[:k] = np.array(vals[:k])
    k = min(n, len(F32S))
    f32[:k] = np.array(F32S[:k], dtype=np.float32)
    nn = (lambda: rng.random(n) >= null_p) if null_p else (lambda: None)
    return Chunk([Column(abi.I64, iv, nn()), Column(abi.U64, uv, nn()), Column(abi.F64, fv, nn()), Column(abi.F32, f32, nn())])


def check(ctx, orc, chk, ids, flags=None, want_chunk=None):
    want, woffs = orc.rowcodec_encode(want_chunk or chk, ids)
    got, offs = RC.Encoder().Encode(ctx, chk, ids, flags)
    assert got.size == want.size and bytes(got) == bytes(want)
    assert (offs == woffs).all()
    return got, offs


# 338 949 rows = 1325 tiles: over the 1024-workgroup cap, so a workgroup owns two tiles and the last one owns one
@pytest.mark.parametrize("n", [0, 1, 255, 256, 257, 4133, 338_949])
def test_rows_equal_the_oracle_at_tile_boundaries(ctx, orc, n):
    rng = np.random.default_rng(n)
    chk = fixed_chunk(rng, n)
    check(ctx, orc, Chunk(chk.columns[:3]), [1, 2, 3])


@pytest.mark.parametrize("ids", [[7, 300, 200, 31], [255], [256], [3, 1, 2, 0], [(1 << 32) - 1, 0]])
def test_id_orders_and_large_by_id(ctx, orc, ids):
    rng = np.random.default_rng(len(ids) + ids[0] % 1000)
    chk = fixed_chunk(rng, 4133)
    check(ctx, orc, Chunk(chk.columns[:len(ids)]), ids)


def test_sixteen_columns(ctx, orc):
    rng = np.random.default_rng(16)
    cols = []
    for _ in range(4):
        cols += fixed_chunk(rng, 1000, null_p=0.3).columns
    for ids in (list(rng.permutation(16) + 1), [int(x) for x in rng.permutation(16) * 40]):  # small, and large by id (wider than the image)
        check(ctx, orc, Chunk(cols), [int(i) for i in ids])


def test_every_fixed_type_at_its_width_edges(ctx, orc):
    n = len(SIGNED)
    chk = fixed_chunk(np.random.default_rng(1), n, null_p=0)
    got, offs = check(ctx, orc, chk, [1, 2, 3, 4])
    assert int(chk.columns[0].data[6]) == -129 and int(chk.columns[1].data[8]) == (1 << 64) - 1


@pytest.mark.parametrize("pattern", ["none", "all", "alternating", "column"])
def test_null_patterns(ctx, orc, pattern):
    n = 4133
    rng = np.random.default_rng(4)
    base = fixed_chunk(rng, n, null_p=0)
    nn = {"none": lambda c: None, "all": lambda c: np.zeros(n, bool), "alternating": lambda c: (np.arange(n) + c) % 2 == 0,
          "column": lambda c: np.zeros(n, bool) if c == 1 else None}[pattern]
    chk = Chunk([Column(col.tp, col.data, nn(c)) for c, col in enumerate(base.columns)])
    check(ctx, orc, chk, [7, 300, 200, 31])
    check(ctx, orc, chk, [4, 3, 2, 1])


def string_rows(rng, n, long_at=()):
    cells = []
    for i in range(n):
        r = rng.random()
        if i in long_at:
            cells.append(bytes(rng.integers(0, 256, 70_000, dtype=np.uint8)))
        elif r < 0.1:
            cells.append(None)
        elif r < 0.3:
            cells.append(b"")
        elif r < 0.5:
            cells.append(bytes([int(rng.integers(0, 256))]))
        elif r < 0.95:
            cells.append(bytes(rng.integers(0, 256, int(rng.integers(2, 40)), dtype=np.uint8)))
        else:
            cells.append(bytes(rng.integers(0, 256, int(rng.integers(64, 230)), dtype=np.uint8)))
    return cells


@pytest.mark.parametrize("wave_copy", [None, 0, 1])
def test_string_columns_staged_and_direct_tiles_in_one_launch(ctx, orc, wave_copy):
    # tile 1 holds a 70 KB cell and is written directly; tiles 0 and 2 go through the LDS image.  wave_copy: the default threshold, never,
    # every cell
    if wave_copy is not None:
        ctx.set_knob(abi.KNOB_ROWENC_WAVE_COPY, wave_copy)
    rng = np.random.default_rng(70)
    n = 768
    fx = fixed_chunk(rng, n)
    chk = Chunk([fx.columns[0], StrColumn(string_rows(rng, n, long_at=(300,))), fx.columns[2], StrColumn(string_rows(rng, n))])
    check(ctx, orc, chk, [1, 2, 3, 4])
    check(ctx, orc, chk, [9, 400, 3, 1])


@pytest.mark.parametrize("wave_copy", [None, 0])
def test_rows_of_65534_65535_65536_value_bytes(ctx, orc, wave_copy):
    # 65535 and more make the row large; at EXACTLY 65535 the reference leaves the 32-bit offsets unset — this project (and its
    # oracle) writes the offsets it means
    if wave_copy is not None:
        ctx.set_knob(abi.KNOB_ROWENC_WAVE_COPY, wave_copy)
    rng = np.random.default_rng(65535)
    totals = [65534, 65535, 65536, 10]
    cells = [bytes(rng.integers(0, 256, t - 1, dtype=np.uint8)) for t in totals]
    chk = Chunk([Column(abi.I64, np.array([5, 6, 7, 8])), StrColumn(cells)])
    got, offs = check(ctx, orc, chk, [1, 2])
    assert [int(got[offs[r] + 1]) for r in range(4)] == [0, 1, 1, 0]
    back = RC.NewChunkDecoder(ctx, [RC.ColInfo(1, RC.TypeLonglong), RC.ColInfo(2, RC.TypeVarchar)]).DecodeToChunk(got, offs)
    assert back.rows() == chk.rows()


@pytest.mark.parametrize("size", [1, 3, 8])
def test_bit_columns(ctx, orc, size):
    rng = np.random.default_rng(size)
    n = 1000
    ints = [int(x) >> int(s) for x, s in zip(rng.integers(0, 1 << (8 * size - 1), n), rng.integers(0, 8 * size, n))]
    ints[:3] = [0, (1 << (8 * size)) - 1, 255]
    nn = rng.random(n) > 0.1
    cells = [v.to_bytes(size, "big") if ok else None for v, ok in zip(ints, nn)]
    fx = fixed_chunk(rng, n)
    chk = Chunk([fx.columns[0], StrColumn(cells)])
    as_uint = Chunk([fx.columns[0], Column(abi.U64, np.array(ints, dtype=np.uint64), nn)])
    flags = [0, abi.RC_BIT | (size << 8)]
    got, offs = check(ctx, orc, chk, [1, 2], flags=flags, want_chunk=as_uint)
    back = RC.NewChunkDecoder(ctx, [RC.ColInfo(1, RC.TypeLonglong), RC.ColInfo(2, RC.TypeBit, Flen=8 * size)]).DecodeToChunk(got, offs)
    assert back.rows() == chk.rows()


def test_bit_cell_of_nine_bytes_is_invalid(ctx):
    chk = Chunk([StrColumn([b"\x01", b"\x01" * 9, b"\x02"])])
    with pytest.raises(_lib.TsqError) as e:
        RC.Encoder().Encode(ctx, chk, [1], [abi.RC_BIT | (8 << 8)])
    assert e.value.status == abi.ERR_INVALID
    with pytest.raises(_lib.TsqError) as e:
        RC.Encoder().Encode(ctx, Chunk([StrColumn([b""])]), [1], [abi.RC_BIT | (1 << 8)])
    assert e.value.status == abi.ERR_INVALID


@pytest.mark.parametrize("phase", [0, 1, 7, 8, 15])
def test_device_resident_columns_and_output_at_every_alignment(ctx, orc, phase):
    rng = np.random.default_rng(40 + phase)
    n = 3000
    fx = fixed_chunk(rng, n, null_p=0.1)
    chk = Chunk(fx.columns + [StrColumn(string_rows(rng, n))])
    ids = [1, 2, 3, 4, 5]
    want, woffs = orc.rowcodec_encode(chk, ids)
    dchk = DeviceChunk.from_host(ctx, chk)
    dout, doffs = ctx.alloc(want.size + phase + 64), ctx.alloc(8 * (n + 1) + 64)
    try:
        ctx.memset(dout, 0xEE, want.size + phase + 64)
        m = C.c_int64(0)
        _lib.check(ctx.lib.tsq_rowcodec_encode(ctx.h, dchk.cols(), 5, (C.c_int64 * 5)(*ids), None, n, C.c_void_p(dout + phase), want.size, abi.COL_DEVICE,
                                               C.c_void_p(doffs), C.byref(m)), ctx.h)
        assert m.value == want.size
        raw = np.zeros(want.size + phase + 64, np.uint8)
        ctx.d2h(raw, dout)
        assert (raw[:phase] == 0xEE).all() and (raw[phase + want.size:] == 0xEE).all() and (raw[phase:phase + want.size] == want).all()
        offs = np.zeros(n + 1, np.int64)
        ctx.d2h(offs, doffs)
        assert (offs == woffs).all()
        # the mirror's device form
        out = RC.Encoder().Encode(ctx, dchk, ids)
        try:
            g, o = out.to_host()
            assert bytes(g) == bytes(want) and (o == woffs).all()
        finally:
            out.free()
    finally:
        ctx.free(dout)
        ctx.free(doffs)
        dchk.free()


def test_round_trip_through_the_decoder(ctx, orc):
    rng = np.random.default_rng(8)
    n = 20_000
    fx = fixed_chunk(rng, n, nan=False)
    chk = Chunk(fx.columns + [StrColumn(string_rows(rng, n))])
    got, offs = RC.Encoder().Encode(ctx, chk, [10, 2, 300, 4, 1])
    infos = [RC.ColInfo(10, RC.TypeLonglong), RC.ColInfo(2, RC.TypeLonglong, RC.UnsignedFlag), RC.ColInfo(300, RC.TypeDouble), RC.ColInfo(4, RC.TypeFloat),
             RC.ColInfo(1, RC.TypeVarchar)]
    back = RC.NewChunkDecoder(ctx, infos).DecodeToChunk(got, offs)
    assert back.rows() == chk.rows()  # a float32 comes back through its double image: exactly


def test_contracts(ctx, orc):
    lib = ctx.lib
    chk = Chunk([Column(abi.I64, np.array([5, 600, 7])), Column(abi.I64, np.array([1, 2, 3]))])
    want, _ = orc.rowcodec_encode(chk, [1, 2])
    keep = []
    cols = make_cols(chk.columns, keep)
    ids = (C.c_int64 * 2)(1, 2)
    out = np.full(256, 0xEE, np.uint8)
    po = out.ctypes.data_as(C.c_void_p)
    m = C.c_int64(-1)
    # nothing to encode is not an error
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, ids, None, 0, po, 256, 0, None, C.byref(m)) == abi.OK and m.value == 0
    # cap_bytes = 0 only asks for the size
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, ids, None, 3, None, 0, 0, None, C.byref(m)) == abi.ERR_INVALID and m.value == want.size
    # one byte short: the size is reported and nothing is written
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, ids, None, 3, po, want.size - 1, 0, None, C.byref(m)) == abi.ERR_INVALID
    assert m.value == want.size and (out == 0xEE).all()
    # misuse
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, ids, None, 3, po, 256, 0, None, None) == abi.ERR_INVALID
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 0, ids, None, 3, po, 256, 0, None, C.byref(m)) == abi.ERR_INVALID
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 17, ids, None, 3, po, 256, 0, None, C.byref(m)) == abi.ERR_INVALID
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, (C.c_int64 * 2)(4, 4), None, 3, po, 256, 0, None, C.byref(m)) == abi.ERR_INVALID  # duplicate id
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, (C.c_int64 * 2)(-1, 4), None, 3, po, 256, 0, None, C.byref(m)) == abi.ERR_INVALID  # negative id
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, (C.c_int64 * 2)(1 << 32, 4), None, 3, po, 256, 0, None, C.byref(m)) == abi.ERR_INVALID
    assert lib.tsq_rowcodec_encode(ctx.h, cols, 2, ids, None, 4, po, 256, 0, None, C.byref(m)) == abi.ERR_INVALID  # column shorter than nrows
    assert (out == 0xEE).all()
    offs = np.zeros(4, np.int64)
    _lib.check(lib.tsq_rowcodec_encode(ctx.h, cols, 2, ids, None, 3, po, 256, 0, offs.ctypes.data_as(C.c_void_p), C.byref(m)), ctx.h)
    assert m.value == want.size and bytes(out[:m.value]) == bytes(want) and (out[m.value:] == 0xEE).all() and offs[3] == want.size
