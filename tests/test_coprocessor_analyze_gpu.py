"""GPU: the two handlers of an ANALYZE coprocessor request (tinysql_amd/coprocessor.py: handleAnalyzeColumnsReq, handleAnalyzeIndexReq)
over a small table built with the oracle's rowcodec / index-key encoders, against tests/analyze_ref.py applied to the oracle's decoded
values.  Two regions merged on the host equal one region over all rows."""
import numpy as np
import pytest

from tests import analyze_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import coprocessor as cop
from tinysql_amd import rowcodec as RC
from tinysql_amd.chunk import Chunk, Column, StrColumn

pytestmark = pytest.mark.gpu

N = 2000
COLS = [RC.ColInfo(-1, RC.TypeLonglong, 0, True), RC.ColInfo(1, RC.TypeLonglong), RC.ColInfo(2, RC.TypeDouble), RC.ColInfo(3, RC.TypeVarchar)]
TYPES = [abi.I64, abi.F64, abi.BYTES]
DEPTH, WIDTH, SKETCH, BUCKETS = 5, 2048, 1000, 64


@pytest.fixture(scope="module")
def table(orc):
    """(pairs of the whole table, its columns as the oracle decodes them, the handles)"""
    rng = np.random.default_rng(5)
    handles = np.sort(rng.choice(np.arange(-5 * N, 5 * N), N, replace=False)).astype(np.int64)
    words = [None if rng.random() < 0.1 else b"w%d" % int(rng.integers(0, 300)) + b"x" * int(rng.integers(0, 20)) for _ in range(N)]
    t = Chunk([Column(abi.I64, rng.integers(-40, 400, N), rng.random(N) >= 0.05), Column(abi.F64, np.round(rng.standard_normal(N) * 10, 1), rng.random(N) >= 0.05),
               StrColumn(words)])
    vals, offs = orc.rowcodec_encode(t, [1, 2, 3])
    st, dec = orc.rowcodec_decode_chunk(vals, offs, handles, [(1, abi.I64), (2, abi.F64), (3, abi.BYTES)])
    assert st == 0 and dec.rows() == t.rows()
    keys = b"".join(orc.encode_row_key(41, int(h)) for h in handles)
    return (keys, vals, offs), [c.values() for c in dec.columns], handles.tolist()


def region(pairs, lo, hi):
    keys, vals, offs = pairs
    return keys[19 * lo:19 * hi], vals[offs[lo]:offs[hi]], offs[lo:hi + 1] - offs[lo]


def check_collector(got, tp, vals, samples):
    want = R.collect(tp, vals, wrap=True, depth=DEPTH, width=WIDTH, max_fm=SKETCH, max_samples=samples, seed=7)
    assert (got.NullCount, got.Count, got.TotalSize) == (want["null_count"], want["count"], want["total_size"])
    assert (got.FMSketch.mask, sorted(got.FMSketch.hashset)) == (want["fm_mask"], want["fm"])
    assert got.CMSketch.count == want["cm_count"] and (got.CMSketch.table == want["cm"]).all()
    return want


@pytest.mark.parametrize("samples", [10, 5000])
def test_analyze_columns(ctx, table, samples):
    pairs, cols, handles = table
    resp = cop.handleAnalyzeColumnsReq(ctx, COLS, pairs, BUCKETS, samples, SKETCH, DEPTH, WIDTH, seed=7, batch_rows=1 << 10)
    wb, wndv = R.sorted_builder_rows(handles, BUCKETS)
    h = resp.PkHist
    assert h.NDV == wndv == N and h.TotalRowCount() == N
    assert [(b.Count, b.Repeat) for b in h.Buckets] == [(b[0], b[1]) for b in wb]
    assert h.lower == [handles[b[2]] for b in wb] and h.upper == [handles[b[3]] for b in wb]
    assert len(resp.Collectors) == 3
    for got, tp, vals in zip(resp.Collectors, TYPES, cols):
        want = check_collector(got, tp, vals, samples)
        assert got.Ordinals == want["sample_ordinals"] and got.Samples == want["samples"]
        if samples > N:
            assert got.Samples == [v for v in vals if v is not None]


def test_two_regions_merged_equal_one(ctx, table):
    pairs, cols, _ = table
    cut = 777
    a = cop.handleAnalyzeColumnsReq(ctx, COLS, region(pairs, 0, cut), BUCKETS, 5000, SKETCH, DEPTH, WIDTH, seed=7)
    b = cop.handleAnalyzeColumnsReq(ctx, COLS, region(pairs, cut, N), BUCKETS, 5000, SKETCH, DEPTH, WIDTH, seed=7)
    assert a.PkHist.TotalRowCount() + b.PkHist.TotalRowCount() == N
    for ca, cb, tp, vals in zip(a.Collectors, b.Collectors, TYPES, cols):
        ca.MergeSampleCollector(cb)
        check_collector(ca, tp, vals, 5000)
        assert ca.Samples == [v for v in vals if v is not None]  # both regions hold all of their rows


def test_without_pk_handle_and_without_cm(ctx, table):
    pairs, cols, _ = table
    resp = cop.handleAnalyzeColumnsReq(ctx, COLS[1:], pairs, BUCKETS, 0, SKETCH)
    assert resp.PkHist is None and len(resp.Collectors) == 3
    for got, tp, vals in zip(resp.Collectors, TYPES, cols):
        want = R.collect(tp, vals, wrap=True, max_fm=SKETCH)
        assert got.CMSketch is None and got.Samples == []
        assert (got.Count, got.NullCount, got.FMSketch.mask, sorted(got.FMSketch.hashset)) == (want["count"], want["null_count"], want["fm_mask"], want["fm"])


@pytest.fixture(scope="module")
def index(orc):
    """a non-unique index on (k int, s varchar), its pairs in key order, and the oracle's decoded index columns"""
    rng = np.random.default_rng(6)
    k = [None if rng.random() < 0.05 else int(rng.integers(0, 40)) for _ in range(N)]
    s = [None if rng.random() < 0.05 else b"name-%02d" % int(rng.integers(0, 30)) + b"-long-tail" * int(rng.integers(0, 3)) for _ in range(N)]
    chunk = Chunk([Column(abi.I64, [0 if v is None else v for v in k], [v is not None for v in k]), StrColumn(s)])
    handles = np.arange(N, dtype=np.int64) * 3 + 1
    keys, offs = orc.encode_index_keys(chunk, 41, 2, handles, np.ones(N, np.uint8))
    raw = [bytes(keys[offs[i]:offs[i + 1]]) for i in range(N)]
    order = sorted(range(N), key=lambda i: raw[i])
    skeys = b"".join(raw[i] for i in order)
    soffs = np.concatenate([[0], np.cumsum([len(raw[i]) for i in order])]).astype(np.int64)
    st, dec = orc.decode_index_kv(skeys, soffs, None, None, 2, [abi.I64, abi.BYTES], 0)
    assert st == 0 and dec.NumRows() == N
    return skeys, soffs, [c.values() for c in dec.columns]


def index_prefixes(cols):
    p1 = [R.encode_datum(abi.I64, v, comparable=True) for v in cols[0]]
    p2 = [a + R.encode_datum(abi.BYTES, v, comparable=True) for a, v in zip(p1, cols[1])]
    return p1, p2


def test_analyze_index(ctx, index):
    skeys, soffs, cols = index
    resp = cop.handleAnalyzeIndexReq(ctx, [abi.I64, abi.BYTES], 2, skeys, soffs, BUCKETS, DEPTH, WIDTH, batch_rows=1 << 10)
    p1, p2 = index_prefixes(cols)
    for i in range(N):  # the prefix is the piece of the key behind its 19-byte header
        assert skeys[soffs[i] + 19:soffs[i] + 19 + len(p2[i])] == p2[i]
    wb, wndv = R.sorted_builder_rows(p2, BUCKETS)
    h = resp.Hist
    assert h.NDV == wndv and h.TotalRowCount() == N
    assert [(b.Count, b.Repeat) for b in h.Buckets] == [(b[0], b[1]) for b in wb]
    assert h.lower == [p2[b[2]] for b in wb] and h.upper == [p2[b[3]] for b in wb]
    assert resp.Cms.count == 2 * N and (resp.Cms.table == R.cm_sketch(p1 + p2, DEPTH, WIDTH)).all()


def test_index_regions_merged_and_no_cm(ctx, index):
    skeys, soffs, cols = index
    cut = 901
    a = cop.handleAnalyzeIndexReq(ctx, [abi.I64, abi.BYTES], 2, skeys[:soffs[cut]], soffs[:cut + 1], BUCKETS, DEPTH, WIDTH)
    b = cop.handleAnalyzeIndexReq(ctx, [abi.I64, abi.BYTES], 2, skeys[soffs[cut]:], soffs[cut:] - soffs[cut], BUCKETS, DEPTH, WIDTH)
    a.Cms.MergeCMSketch(b.Cms)
    p1, p2 = index_prefixes(cols)
    assert a.Cms.count == 2 * N and (a.Cms.table == R.cm_sketch(p1 + p2, DEPTH, WIDTH)).all()
    one = cop.handleAnalyzeIndexReq(ctx, [abi.I64, abi.BYTES], 1, skeys, soffs, 3)
    wb, wndv = R.sorted_builder_rows(p1, 3)
    assert one.Cms is None and one.Hist.NDV == wndv and [(x.Count, x.Repeat) for x in one.Hist.Buckets] == [(x[0], x[1]) for x in wb]
    assert one.Hist.upper == [p1[x[3]] for x in wb]
