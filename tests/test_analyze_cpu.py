"""CPU: pins tests/analyze_ref.py — the restatement the GPU ANALYZE tests compare with — on published murmur3 vectors, on the
reference's own FM sketch values (statistics/fmsketch_test.go:36-47 over the data of statistics_test.go:109-166) and on the row-by-row
SortedBuilder; and the new entry points of the C-ABI."""
import ctypes as C
import os
import random
import subprocess

import pytest

from tests import analyze_ref as R
from tinysql_amd import _abi as abi

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.mark.parametrize("text,h1,h2", [
    (b"", 0, 0),
    (b"hello", 0xcbd8a7b341bd9b02, 0x5b1e906a48ae1d19),
    (b"hello, world", 0x342fac623a5ebc8e, 0x4cdcbc079642414d),
    (b"The quick brown fox jumps over the lazy dog.", 0xcd99481f9ee902c9, 0x695da1a38987b6e7),
])
def test_murmur3_128_vectors(text, h1, h2):
    assert R.murmur3_128(text) == (h1, h2)
    assert R.murmur3_64(text) == h1


def test_datum_bytes():
    assert R.encode_datum(R.I64, 0) == b"\x08\x00"
    assert R.encode_datum(R.I64, -1) == b"\x08\x01"
    assert R.encode_datum(R.I64, 64) == b"\x08\x80\x01"
    assert len(R.encode_datum(R.I64, -(1 << 63))) == 11
    assert R.encode_datum(R.U64, 300) == b"\x09\xac\x02"
    assert R.encode_datum(R.I64, 1, comparable=True) == b"\x03\x80\x00\x00\x00\x00\x00\x00\x01"
    assert R.encode_datum(R.F64, 0.0) == b"\x05\x80" + b"\x00" * 7
    assert R.encode_datum(R.BYTES, b"abc") == b"\x02\x06abc"
    assert R.encode_datum(R.BYTES, b"abc", comparable=True) == b"\x01abc\x00\x00\x00\x00\x00\xfa"
    assert R.encode_datum(R.BYTES, b"", comparable=True) == b"\x01" + b"\x00" * 8 + b"\xf7"
    assert R.wrap_bytes(b"\x08\x02") == b"\x02\x04\x08\x02"


@pytest.fixture(scope="module")
def ref_hashes():
    return {name: [R.murmur3_64(R.encode_datum(R.I64, v)) for v in data]
            for name, data in (("samples", R.ref_samples()), ("rc", R.ref_rc()), ("pk", R.ref_pk()))}


@pytest.mark.parametrize("name,ndv,mask,entries", [("samples", 6232, 7, 779), ("rc", 73344, 127, 573), ("pk", 100480, 127, 785)])
def test_reference_fm_vectors(ref_hashes, name, ndv, mask, entries):
    # maxSize 1000, unwrapped int datums: this also confirms the varint datum encoding
    seq = R.fm_sequential(ref_hashes[name], 1000)
    can = R.fm_canonical(ref_hashes[name], 1000)
    assert seq == can
    assert (R.fm_ndv(can), can[0], len(can[1])) == (ndv, mask, entries)


def test_reference_fm_merge(ref_hashes):
    sk = [R.fm_canonical(ref_hashes[n], 1000) for n in ("samples", "pk", "rc")]
    m = R.fm_merge(R.fm_merge(sk[0], sk[1], 1000), sk[2], 1000)
    assert R.fm_ndv(m) == 100480
    assert m == R.fm_canonical(ref_hashes["samples"] + ref_hashes["pk"] + ref_hashes["rc"], 1000)


@pytest.mark.parametrize("max_size", [1, 2, 3, 7])
def test_sequential_equals_canonical_within_the_limit(max_size):
    # the reference can end above its own limit when no passing value follows the last doubling: only then the two differ
    rng = random.Random(max_size)
    over = 0
    for _ in range(100):
        hs = [rng.getrandbits(64) >> rng.randrange(0, 60) << rng.randrange(0, 6) for _ in range(rng.randrange(0, 40))]
        seq, can = R.fm_sequential(hs, max_size), R.fm_canonical(hs, max_size)
        assert len(can[1]) <= max_size
        if len(seq[1]) <= max_size:
            assert seq == can
        else:
            over += 1
            assert seq != can
    assert over < 100


def test_sorted_builder_run_jump_equals_row_by_row():
    rng = random.Random(7)
    for trial in range(3000):
        n = rng.randrange(0, 120)
        ndv = rng.choice([1, 2, 5, 30, 1000])
        vals = [rng.randrange(ndv) for _ in range(n)]
        if trial % 5:
            vals.sort()  # (an unsorted input is legal: the builder only compares neighbours)
        nb = rng.randrange(1, 17)
        rows = R.sorted_builder_rows(vals, nb) if n else ([], 0)
        assert R.sorted_builder_runs(vals, nb) == rows, (vals, nb)


def test_sorted_builder_values_of_the_reference_data():
    # this project's values (the reference pins only the count and Repeat > 0, statistics_test.go:230-234, 293, 310)
    b, ndv = R.sorted_builder_runs(R.ref_pk(), 256)
    assert (len(b), b[-1], ndv) == (196, [100000, 1, 99840, 99999], 100000)
    rc = R.ref_rc()
    b, ndv = R.sorted_builder_runs(rc, 256)
    assert (len(b), b[0][:2], rc[b[0][2]], rc[b[0][3]], ndv) == (193, [1620, 2], 0, 1619, 72602)
    assert b == R.sorted_builder_rows(rc, 256)[0]


def test_sampler_takes_every_row_up_to_its_size():
    nn = [i % 3 != 0 for i in range(50)]
    assert R.sample_ordinals(nn, 9, 100) == [i for i in range(50) if nn[i]]
    s = R.sample_ordinals(nn, 9, 10)
    assert len(s) == 10 and s == sorted(s) and all(nn[i] for i in s)
    assert R.sample_ordinals(nn, 9, 0) == []


def test_new_abi_is_declared_and_the_version_stays():
    assert abi.TSQ_ABI_VERSION == 10
    for name in ("tsq_analyze_create", "tsq_analyze_push", "tsq_analyze_finish", "tsq_analyze_cancel", "tsq_analyze_destroy", "tsq_analyze_column",
                 "tsq_analyze_fm", "tsq_analyze_cm", "tsq_analyze_samples", "tsq_analyze_samples_peek", "tsq_analyze_stats", "tsq_sorted_hist_create",
                 "tsq_sorted_hist_push", "tsq_sorted_hist_finish", "tsq_sorted_hist_peek", "tsq_sorted_hist_result", "tsq_sorted_hist_stats",
                 "tsq_sorted_hist_destroy"):
        assert name in abi.SIGNATURES
    assert C.sizeof(abi.AnalyzeCfg) == 176


def test_analyze_cfg_size_equals_what_gcc_computes(tmp_path):
    src = tmp_path / "sz.c"
    src.write_text('#include <stdio.h>\n#include <stddef.h>\n#include "%s"\nint main(){printf("%%zu %%zu %%zu\\n", sizeof(tsq_analyze_cfg), '
                   'offsetof(tsq_analyze_cfg, max_sample_size), offsetof(tsq_analyze_cfg, sample_seed));return 0;}\n' % os.path.join(ROOT, "include", "tsq.h"))
    exe = tmp_path / "sz"
    subprocess.run(["gcc", str(src), "-o", str(exe)], check=True)
    got = [int(x) for x in subprocess.run([str(exe)], check=True, capture_output=True, text=True).stdout.split()]
    assert got == [C.sizeof(abi.AnalyzeCfg), abi.AnalyzeCfg.max_sample_size.offset, abi.AnalyzeCfg.sample_seed.offset]


def dp_cases():
    """(type, col_flags, value): the edge values of the GPU test, every datum length 2..11 and every string length around the block size"""
    ints = [0, 1, -1, 64, -64, 1 << 13, -(1 << 13), 1 << 62, -(1 << 63), (1 << 63) - 1, 123456789]
    out = [(abi.I64, f, v) for v in ints for f in (0, abi.ENC_COMPARABLE)]
    out += [(abi.U64, f, v) for v in (0, 1, 127, 128, (1 << 63) + 5, (1 << 64) - 1) for f in (0, abi.ENC_COMPARABLE)]
    out += [(abi.F64, 0, v) for v in (0.0, -0.0, 1.5, -2.25, 1e300, float("inf"))]
    out += [(abi.F32, 0, v) for v in (0.0, 1.5, -3.75)]
    for n in (0, 1, 7, 8, 9, 15, 16, 17, 31, 32, 33, 100):
        cell = bytes((i * 37 + n) & 0xff for i in range(n))
        out += [(abi.BYTES, f, cell) for f in (0, abi.ENC_COMPARABLE, abi.AN_RAW)]
    return out


def test_device_header_on_the_host_equals_the_restatement(tmp_path):
    import struct
    exe = tmp_path / "analyze_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "analyze_dp_main.cpp"), "-o", str(exe)], check=True)
    lines, want = [], []
    for tp, flags, v in dp_cases():
        if tp == abi.BYTES:
            text = v.hex() or "-"
            e = v if flags & abi.AN_RAW else R.encode_datum(tp, v, bool(flags & abi.ENC_COMPARABLE))
        else:
            if tp == abi.F64:
                bits = struct.unpack("<Q", struct.pack("<d", v))[0]
            elif tp == abi.F32:
                bits = struct.unpack("<I", struct.pack("<f", v))[0]
            else:
                bits = v & R.M64
            text = str(bits)
            e = R.encode_datum(tp, v, bool(flags & abi.ENC_COMPARABLE))
        lines.append("%d %d 0 %s" % (tp, flags, text))
        h1, h2 = R.murmur3_128(e)
        want.append((len(e), h1, h2, h1, R.murmur3_64(R.wrap_bytes(e))))
    res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
    assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
    got = [tuple([int(f[0])] + [int(x, 16) for x in f[1:]]) for f in (ln.split() for ln in res.stdout.splitlines())]
    assert got == want
