"""GPU parity of tsq_indexkeys_encode (chunk rows -> index entries: index.GenIndexKey + the value index.Create stores,
table/tables/index.go:161-244) against the oracle's restatement of EncodeIndexSeekKey + EncodeKey: byte-identical keys and key
boundaries, the values / value boundaries / distinct flags against their definition, the round trip through tsq_indexkeys_decode,
device placement, and index prefix lengths (TruncateIndexValuesIfNeeded, :127-157) in both charsets."""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import coprocessor as cop
from tinysql_amd import tablecodec as TC
from tinysql_amd.chunk import Chunk, Column, StrColumn
from tinysql_amd.gpu_pipeline import DeviceChunk, drain_device

pytestmark = pytest.mark.gpu

STR_LENS = [0, 7, 8, 9, 16, 200]


def col_of(rng, tp, n, null_p=0.1):
    nn = rng.random(n) >= null_p if null_p else None
    if tp == abi.I64:
        return Column(tp, rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64) >> rng.integers(0, 64, n), nn)
    if tp == abi.U64:
        return Column(tp, rng.integers(0, (1 << 64) - 1, n, dtype=np.uint64) >> rng.integers(0, 64, n).astype(np.uint64), nn)
    if tp == abi.F64:
        v = np.ldexp(rng.random(n) - 0.5, rng.integers(-60, 60, n))
        v[:min(n, 4)] = np.array([0.0, -0.0, np.inf, -np.inf])[:min(n, 4)]
        return Column(tp, v, nn)
    cells = [None if (nn is not None and not nn[i]) else bytes(rng.integers(0, 256, STR_LENS[int(rng.integers(0, len(STR_LENS)))], dtype=np.uint8)) for i in range(n)]
    return StrColumn(cells)


def want_entries(orc, chk, tid, iid, handles, unique):
    """(keys, key_offsets, values, value_offsets, distinct) by definition"""
    n = chk.NumRows()
    has_null = np.array([any(c.IsNull(r) for c in chk.columns) for r in range(n)], dtype=bool)
    in_key = has_null if unique else np.ones(n, bool)
    keys, koffs = orc.encode_index_keys(chk, tid, iid, handles, in_key.astype(np.uint8))
    parts = [b"0" if k else int(h).to_bytes(8, "big", signed=True) for h, k in zip(handles, in_key)]
    voffs = np.concatenate([[0], np.cumsum([len(p) for p in parts])]).astype(np.int64)
    return keys, koffs, b"".join(parts), voffs, (~in_key).astype(np.uint8)


def check(ctx, orc, chk, tid, iid, handles, unique, prefix_len=None, prefix_utf8=None, want_chunk=None):
    wk, wko, wv, wvo, wd = want_entries(orc, want_chunk or chk, tid, iid, handles, unique)
    keys, ko, vals, vo, dist = TC.GenIndexKeys(ctx, tid, iid, unique, chk, handles, prefix_len, prefix_utf8)
    assert bytes(keys) == bytes(wk) and (ko == wko).all()
    assert bytes(vals) == wv and (vo == wvo).all() and (dist == wd).all()
    return keys, ko, vals, vo


@pytest.mark.parametrize("types", [(abi.I64,), (abi.U64, abi.F64), (abi.I64, abi.BYTES), (abi.BYTES, abi.BYTES)])
@pytest.mark.parametrize("n", [0, 1, 256, 257, 4133])
def test_entries_against_the_oracle_and_back_through_the_decoder(ctx, orc, n, types):
    rng = np.random.default_rng(n + 10 * len(types) + types[0])
    chk = Chunk([col_of(rng, t, n) for t in types])
    handles = rng.integers(-(1 << 62), 1 << 62, n)
    handles[:min(n, 3)] = np.array([-1, -(1 << 63), (1 << 63) - 1])[:min(n, 3)]
    for unique in (False, True):
        keys, ko, vals, vo = check(ctx, orc, chk, 45, 3, handles, unique)
        if n == 0:
            continue
        itypes = list(types) + [abi.I64]
        scan = cop.indexScanExec(ctx, itypes, len(types), cop.indexScanExec.PrimaryKeyIsSigned, keys, ko, vals, vo)
        rows = [r for ch in drain_device(scan) for r in ch.rows()]
        assert [r[:-1] for r in rows] == chk.rows() and [r[-1] for r in rows] == handles.tolist()


@pytest.mark.parametrize("tid,iid", [(-(1 << 63), (1 << 63) - 1), ((1 << 63) - 1, -(1 << 63)), (0, -1)])
def test_table_and_index_id_extremes(ctx, orc, tid, iid):
    rng = np.random.default_rng(5)
    chk = Chunk([col_of(rng, abi.I64, 300), col_of(rng, abi.BYTES, 300)])
    check(ctx, orc, chk, tid, iid, rng.integers(-(1 << 62), 1 << 62, 300), True)


@pytest.mark.parametrize("wave_copy", [0, 1])
def test_long_cells_with_and_without_the_wave_copy(ctx, orc, wave_copy):
    ctx.set_knob(abi.KNOB_ROWENC_WAVE_COPY, wave_copy)
    rng = np.random.default_rng(200)
    n = 700
    cells = [bytes(rng.integers(0, 256, 70_000 if i == 300 else STR_LENS[i % len(STR_LENS)], dtype=np.uint8)) for i in range(n)]  # tile 1 is written directly
    chk = Chunk([col_of(rng, abi.I64, n), StrColumn(cells)])
    check(ctx, orc, chk, 1, 2, np.arange(n, dtype=np.int64) - 350, False)


def test_device_resident_columns_and_outputs(ctx, orc):
    rng = np.random.default_rng(12)
    n = 4133
    chk = Chunk([col_of(rng, abi.I64, n), col_of(rng, abi.BYTES, n)])
    handles = rng.integers(-(1 << 62), 1 << 62, n)
    wk, wko, wv, wvo, wd = want_entries(orc, chk, 9, 4, handles, True)
    dchk = DeviceChunk.from_host(ctx, chk)
    dh = ctx.alloc(8 * n + 64)
    try:
        ctx.h2d(dh, np.ascontiguousarray(handles, dtype=np.int64))
        kvs = TC.GenIndexKeys(ctx, 9, 4, True, dchk, dh)
        try:
            keys, ko, vals, vo, dist = kvs.to_host()
        finally:
            kvs.free()
        assert bytes(keys) == bytes(wk) and (ko == wko).all() and bytes(vals) == wv and (vo == wvo).all() and (dist == wd).all()
    finally:
        ctx.free(dh)
        dchk.free()


TEXTS = ["", "a", "abc", "abcdef", "héllo wörld", "日本語のテキスト", "a日b本c語", "\U0001f600\U0001f601x\U0001f602", "ééééé", "z" * 40]


@pytest.mark.parametrize("k", [0, 1, 3, 100])
def test_prefix_lengths_in_both_charsets(ctx, orc, k):
    # truncate in Python, hand the truncated chunk to the oracle; multi-byte runes straddle the byte cut of the binary column
    n = 600
    cells = [None if i % 17 == 0 else TEXTS[i % len(TEXTS)].encode() for i in range(n)]
    ints = Column(abi.I64, np.arange(n) * 7 - 100)
    handles = np.arange(n, dtype=np.int64)
    chk = Chunk([StrColumn(cells), ints, StrColumn(cells)])
    cut_utf8 = [None if c is None else c.decode()[:k].encode() for c in cells]
    cut_bin = [None if c is None else c[:k] for c in cells]
    want = Chunk([StrColumn(cut_utf8), ints, StrColumn(cut_bin)])
    for unique in (False, True):
        check(ctx, orc, chk, 7, 1, handles, unique, prefix_len=[k, 5, k], prefix_utf8=[1, 1, 0], want_chunk=want)  # (the int column ignores its length)
    check(ctx, orc, chk, 7, 1, handles, False, prefix_len=[-1, -1, -1], prefix_utf8=[1, 0, 0])
    check(ctx, orc, chk, 7, 1, handles, False, prefix_len=None, prefix_utf8=[1, 0, 1])


def test_invalid_utf8_under_a_prefix(ctx, orc):
    bad = [b"ab\xffcd", b"\xc0\x80xyz", b"ok", b"\xe4\xb8", b"abc\xed\xa0\x80"]
    handles = np.arange(len(bad), dtype=np.int64)
    chk = Chunk([StrColumn(bad)])
    # binary charset: simply sliced
    check(ctx, orc, chk, 1, 1, handles, False, prefix_len=[3], prefix_utf8=[0], want_chunk=Chunk([StrColumn([c[:3] for c in bad])]))
    # utf8, the invalid byte behind the cut of every truncated cell: encodes normally (cells 1 and 3 are left out: invalid inside)
    behind = Chunk([StrColumn([bad[0], bad[2], bad[4]])])
    check(ctx, orc, behind, 1, 1, handles[:3], False, prefix_len=[2], prefix_utf8=[1], want_chunk=Chunk([StrColumn([b"ab", b"ok", b"ab"])]))
    # utf8, not truncated (the prefix holds every rune): never touched, valid or not
    check(ctx, orc, chk, 1, 1, handles, True, prefix_len=[8], prefix_utf8=[1])
    # utf8, an invalid byte inside the kept prefix of a truncated cell: the Go path
    for k, cells in ((3, bad), (1, [b"fine", b"\xc0\x80xyz"]), (1, [b"\xe4\xb8"])):
        with pytest.raises(_lib.TsqError) as e:
            TC.GenIndexKeys(ctx, 1, 1, False, Chunk([StrColumn(cells)]), np.arange(len(cells), dtype=np.int64), [k], [1])
        assert e.value.status == abi.ERR_UNSUPPORTED
    # ... but b"\xe4\xb8" under a prefix of two runes is two (invalid) runes: not truncated
    check(ctx, orc, Chunk([StrColumn([b"\xe4\xb8"])]), 1, 1, handles[:1], False, prefix_len=[2], prefix_utf8=[1])


def test_contracts(ctx, orc):
    lib = ctx.lib
    from tinysql_amd.chunk import make_cols
    chk = Chunk([Column(abi.I64, np.array([5, 6, 7]))])
    h = np.array([1, 2, 3], dtype=np.int64)
    wk, wko, wv, wvo, wd = want_entries(orc, chk, 1, 1, h, False)
    keep = []
    cols = make_cols(chk.columns, keep)
    out = np.full(256, 0xEE, np.uint8)
    ko, vo, vals, dist = np.full(4, -1, np.int64), np.full(4, -1, np.int64), np.full(24, 0xEE, np.uint8), np.full(3, 0xEE, np.uint8)
    p = lambda a: a.ctypes.data_as(C.c_void_p)
    m = C.c_int64(-1)
    call = lambda ncols, nrows, outp, cap: lib.tsq_indexkeys_encode(ctx.h, 1, 1, 0, cols, ncols, None, None, p(h), nrows, 0, outp, cap, p(ko), p(vals), p(vo), p(dist),
                                                                    C.byref(m))
    assert call(1, 3, None, 0) == abi.ERR_INVALID and m.value == len(wk)                      # the size question
    assert call(1, 3, p(out), len(wk) - 1) == abi.ERR_INVALID and m.value == len(wk)         # one byte short: nothing written
    assert (out == 0xEE).all() and (vals == 0xEE).all() and (dist == 0xEE).all() and (ko == -1).all() and (vo == -1).all()
    assert call(0, 3, p(out), 256) == abi.ERR_INVALID and call(17, 3, p(out), 256) == abi.ERR_INVALID
    assert call(1, 4, p(out), 256) == abi.ERR_INVALID                                         # column shorter than nrows
    assert call(1, 0, p(out), 256) == abi.OK and m.value == 0 and ko[0] == 0 and vo[0] == 0
    assert call(1, 3, p(out), 256) == abi.OK and m.value == len(wk) and bytes(out[:m.value]) == bytes(wk) and (out[m.value:] == 0xEE).all()
    assert bytes(vals[:3]) == b"000" and (dist == 0).all() and (ko == wko).all() and (vo == wvo).all()
