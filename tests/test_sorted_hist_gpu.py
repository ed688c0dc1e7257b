"""GPU: the histogram of a sorted stream (tsq_sorted_hist_*) against the row-by-row SortedBuilder of tests/analyze_ref.py: bucket
counts, repeats, bounds (as row numbers and as values) and the NDV, exactly."""
import numpy as np
import pytest

from tests import analyze_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Chunk, Column, StrColumn
from tinysql_amd.gpu_pipeline import DeviceChunk
from tinysql_amd.statistics import SortedBuilder

pytestmark = pytest.mark.gpu

BUCKETS = [1, 2, 3, 256]


def build(ctx, tp, values, num_buckets, pushes=None, device=False):
    with SortedBuilder(ctx, tp, num_buckets) as b:
        lo = 0
        for n in pushes or [len(values)]:
            col = StrColumn(values[lo:lo + n]) if tp == abi.BYTES else Column(tp, values[lo:lo + n])
            if device and n:
                dev = DeviceChunk.from_host(ctx, Chunk([col]))
                try:
                    b.push(dev.columns[0], n)
                finally:
                    dev.free()
            else:
                b.push(col)
            lo += n
        h = b.Hist()
        return h, b.Count, b.stats()


def check(ctx, tp, values, num_buckets, want=None, **kw):
    h, count, st = build(ctx, tp, values, num_buckets, **kw)
    wb, wndv = want if want is not None else (R.sorted_builder_rows(values, num_buckets) if values else ([], 0))
    assert count == len(values) and h.NDV == wndv
    assert [(b.Count, b.Repeat) for b in h.Buckets] == [(b[0], b[1]) for b in wb]
    assert h.lower_rows == [b[2] for b in wb] and h.upper_rows == [b[3] for b in wb]
    assert h.lower == [values[b[2]] for b in wb] and h.upper == [values[b[3]] for b in wb]
    return h, st


@pytest.fixture(scope="module")
def ref_hists():
    """the row-by-row builder over the reference's 100 000-row test data, once per bucket count"""
    return {(name, nb): R.sorted_builder_rows(data, nb) for name, data in (("pk", R.ref_pk()), ("rc", R.ref_rc())) for nb in BUCKETS}


@pytest.mark.parametrize("nb", BUCKETS)
@pytest.mark.parametrize("n", [1, 2, 257])
def test_small_inputs(ctx, nb, n):
    rng = np.random.default_rng(n * 31 + nb)
    check(ctx, abi.I64, list(range(n)), nb)
    check(ctx, abi.I64, sorted(int(x) for x in rng.integers(0, max(2, n // 3), n)), nb)


@pytest.mark.parametrize("nb", BUCKETS)
@pytest.mark.parametrize("name", ["pk", "rc"])
def test_reference_data(ctx, ref_hists, name, nb):
    data = R.ref_pk() if name == "pk" else R.ref_rc()
    h, st = check(ctx, abi.I64, data, nb, want=ref_hists[(name, nb)], device=name == "rc")
    if nb == 256:  # this project's values (the reference pins only the count and Repeat > 0)
        if name == "pk":
            assert (h.Len(), h.lower[-1], h.upper[-1], h.Buckets[-1].Count, h.Buckets[-1].Repeat) == (196, 99840, 99999, 100000, 1)
            # a merge epoch fills at most 128 more buckets with one search each, there are log2(N / 128) epochs, the first 256 buckets take one each
            assert st["steps"] <= 128 * np.log2(len(data) / 128) + 256
        else:
            assert (h.Len(), h.lower[0], h.upper[0], h.Buckets[0].Count, h.Buckets[0].Repeat, h.NDV) == (193, 0, 1619, 1620, 2, 72602)


@pytest.mark.parametrize("nb", BUCKETS)
def test_long_run_and_runs_ending_at_wave_boundaries(ctx, nb):
    check(ctx, abi.I64, [4] * 5000, nb)  # one run, longer than a workgroup tile
    check(ctx, abi.I64, [1] * 10 + [4] * 5000 + [9, 9, 11], nb)
    for end in (63, 64, 65):
        check(ctx, abi.I64, [5] * end + [6] * (128 - end) + [7] * end + list(range(8, 40)), nb)


@pytest.mark.parametrize("nb", BUCKETS)
def test_two_pushes_cut_a_run(ctx, nb):
    vals = [1] * 40 + [2] * 100 + [3] * 7 + list(range(4, 300))
    check(ctx, abi.I64, vals, nb, pushes=[90, len(vals) - 90])
    check(ctx, abi.I64, vals, nb, pushes=[90, 0, 50, len(vals) - 140], device=True)


@pytest.mark.parametrize("nb", BUCKETS)
def test_unsigned_above_2_63_and_unsorted_input(ctx, nb):
    vals = sorted([(1 << 63) + i // 3 for i in range(200)] + [5, 5, (1 << 64) - 1, (1 << 64) - 1])
    check(ctx, abi.U64, vals, nb)
    check(ctx, abi.I64, [3, 1, 1, 2, 3, 3, 1] * 20, nb)  # the order is the caller's contract: an unsorted input is no error


@pytest.mark.parametrize("nb", BUCKETS)
def test_bytes_keys_with_long_shared_prefixes(ctx, nb):
    p = b"a-long-shared-prefix-of-an-index-key/" * 3
    vals = sorted([p[:n] for n in range(len(p) - 20, len(p))] * 2 + [p + bytes([i // 4]) for i in range(100)] + [b"", b"", p + b"\x00\x00"])
    check(ctx, abi.BYTES, vals, nb)
    check(ctx, abi.BYTES, vals, nb, pushes=[33, len(vals) - 33], device=True)


def test_empty_input_and_bad_arguments(ctx):
    h, count, _ = build(ctx, abi.I64, [], 256)
    assert (h.Len(), h.NDV, count, h.TotalRowCount()) == (0, 0, 0, 0)
    for tp, nb, status in ((abi.F64, 256, abi.ERR_UNSUPPORTED), (abi.I64, 0, abi.ERR_INVALID), (abi.I64, 5000, abi.ERR_UNSUPPORTED)):
        with pytest.raises(_lib.TsqError) as ei:
            SortedBuilder(ctx, tp, nb)
        assert ei.value.status == status
    with SortedBuilder(ctx, abi.I64, 4) as b:
        b.push(Column(abi.I64, [1, 2]))
        b.Hist()
        with pytest.raises(_lib.TsqError) as ei:
            b.push(Column(abi.I64, [3]))
        assert ei.value.status == abi.ERR_INVALID
