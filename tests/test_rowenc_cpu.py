"""CPU: the per-row arithmetic of the write-path kernels (tinysql_amd/csrc/tsq_rowenc_dp.h, the very code the kernels run, built on
the host as a stand-alone sanitized program) against the oracle's restatement of rowcodec.Encoder.Encode — value widths at their edges,
row length, the `large` decision at 65534 / 65535 / 65536 value bytes and at ids 255 / 256 — and the rune walk of an index prefix
against strict Python decoding and Go's utf8.DecodeRune on invalid input; and the two new entry points of the C-ABI."""
import os
import random
import struct
import subprocess

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Chunk, Column

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))


@pytest.fixture(scope="module")
def dp(tmp_path_factory):
    exe = tmp_path_factory.mktemp("rowenc") / "rowenc_dp"
    subprocess.run(["g++", "-std=c++17", "-O1", "-g", "-fsanitize=address,undefined", "-fno-sanitize-recover=all",
                    os.path.join(ROOT, "tests", "rowenc_dp_main.cpp"), "-o", str(exe)], check=True)

    def run(lines):
        res = subprocess.run([str(exe)], input="\n".join(lines) + "\n", capture_output=True, text=True)
        assert res.returncode == 0, res.stdout[-500:] + res.stderr[-2000:]
        out = res.stdout.splitlines()
        assert len(out) == len(lines)
        return [ln.split() for ln in out]
    return run


def hexs(b):
    return bytes(b).hex() or "-"


SIGNED = [0, 1, -1, 127, 128, -128, -129, 32767, 32768, -32768, -32769, (1 << 31) - 1, 1 << 31, (1 << 31) + 1, -(1 << 31), -(1 << 31) - 1, -(1 << 31) + 1,
          (1 << 63) - 1, -(1 << 63)]
UNSIGNED = [0, 1, 255, 256, 65535, 65536, (1 << 32) - 1, 1 << 32, (1 << 64) - 1]
F64S = [0.0, -0.0, float("nan"), float("inf"), float("-inf"), 1.5, -2.25, 1e300]
F32S = [0.1, -0.1, 1.5, float("inf"), 16777217.0]  # 0.1f widens to 0.100000001490116...


def test_value_bytes_equal_the_oracle_at_every_width_edge(dp, orc):
    cases = [(abi.I64, v, v & ((1 << 64) - 1)) for v in SIGNED] + [(abi.U64, v, v) for v in UNSIGNED]
    cases += [(abi.F64, v, struct.unpack("<Q", struct.pack("<d", v))[0]) for v in F64S]
    cases += [(abi.F32, v, struct.unpack("<I", struct.pack("<f", v))[0]) for v in F32S]
    got = dp(["v %d %d" % (tp, bits) for tp, _, bits in cases])
    for (tp, v, _), g in zip(cases, got):
        data = np.array([v], dtype={abi.I64: np.int64, abi.U64: np.uint64, abi.F64: np.float64, abi.F32: np.float32}[tp])
        row, offs = orc.rowcodec_encode(Chunk([Column(tp, data)]), [1])
        want = bytes(row[9:])  # header 6, one id, one u16 offset
        assert (int(g[0]), g[1]) == (len(want), want.hex()), (tp, v)
        assert offs[1] == 9 + len(want)


@pytest.mark.parametrize("ids", [[1, 2, 3], [255, 7, 9], [256, 7, 9], [7, 300, 200]])
def test_row_length_and_header_equal_the_oracle(dp, orc, ids):
    rng = np.random.default_rng(sum(ids))
    n = 64
    iv = rng.integers(-(1 << 63), (1 << 63) - 1, n, dtype=np.int64) >> rng.integers(0, 64, n)
    chk = Chunk([Column(abi.I64, iv, rng.random(n) > 0.3), Column(abi.U64, (iv & 0xffff).astype(np.uint64), rng.random(n) > 0.3),
                 Column(abi.F64, rng.random(n), rng.random(n) > 0.3)])
    rows, offs = orc.rowcodec_encode(chk, ids)
    lines = []
    for r in range(n):
        nn = [not c.IsNull(r) for c in chk.columns]
        vb = 0
        if nn[0]:
            v = int(iv[r])
            vb += 1 if -128 <= v < 128 else 2 if -(1 << 15) <= v < (1 << 15) else 4 if -(1 << 31) <= v < (1 << 31) else 8
        if nn[1]:
            vb += 1 if int(iv[r]) & 0xffff < 256 else 2
        if nn[2]:
            vb += 8
        lines.append("r %d %d %d %d" % (1 if max(ids) > 255 else 0, sum(nn), 3 - sum(nn), vb))
    got = dp(lines)
    for r in range(n):
        row = bytes(rows[offs[r]:offs[r + 1]])
        assert (int(got[r][0]), int(got[r][1]), got[r][2]) == (row[1], len(row), row[:6].hex()), r


@pytest.mark.parametrize("total", [65534, 65535, 65536])
@pytest.mark.parametrize("first_id", [255, 256])
def test_large_decision_at_the_value_byte_edges(dp, orc, total, first_id):
    # one 1-byte int + a pad cell: `total` value bytes.  At exactly 65535 the oracle (as this project) writes a large row
    chk = Chunk([Column(abi.I64, np.array([5]))])
    rows, offs = orc.rowcodec_encode(chk, [first_id], pad_col_id=3, pad_len=[total - 1])
    row = bytes(rows)
    g = dp(["r %d 2 0 %d" % (1 if first_id > 255 else 0, total)])[0]
    assert (int(g[0]), int(g[1]), g[2]) == (row[1], len(row), row[:6].hex())
    assert int(g[0]) == (1 if first_id > 255 or total >= 65535 else 0)


def test_bit_cells(dp):
    cells = [b"\x01", b"\x00\x01\x02", b"\xff" * 8, b"\x00" * 8, b"", b"\x01" * 9]
    got = dp(["b " + hexs(c) for c in cells])
    want = [(1, int.from_bytes(c, "big")) if 1 <= len(c) <= 8 else (0, 0) for c in cells]
    assert [(int(g[0]), int(g[1])) for g in got] == want


GO_CASES = [(b"\xff", 1), (b"\xc0\x80", 2), (b"\xed\xa0\x80", 3), (b"\xe4\xb8", 2), (b"\xf4\x90\x80\x80", 4)]


def rand_text(rng, n):
    pools = [(0x20, 0x7e), (0x80, 0x7ff), (0x800, 0xd7ff), (0xe000, 0xffff), (0x10000, 0x10ffff)]
    return "".join(chr(rng.randint(*pools[rng.randrange(len(pools))])) for _ in range(n))


def test_rune_walk_counts_like_strict_decoding_and_like_go(dp):
    rng = random.Random(5)
    texts = [rand_text(rng, rng.randrange(0, 40)) for _ in range(200)] + ["", "\u00e9", "\ud7ff", "\ue000", "\U0010ffff", "\ufffd", "\x7f\x80\u07ff\u0800"]
    got = dp(["u " + hexs(t.encode()) for t in texts] + ["u " + hexs(b) for b, _ in GO_CASES])
    assert [int(g[0]) for g in got] == [len(t.encode().decode("utf-8", "strict")) for t in texts] + [n for _, n in GO_CASES]


def test_rune_prefix_keeps_what_python_slicing_keeps(dp):
    rng = random.Random(6)
    lines, want = [], []
    for _ in range(300):
        t = rand_text(rng, rng.randrange(0, 12))
        k = rng.choice([0, 1, 3, 5, 50])
        lines.append("p %d 1 %s" % (k, hexs(t.encode())))
        want.append((len(t[:k].encode()), 0))
        b = t.encode()
        lines.append("p %d 0 %s" % (k, hexs(b)))  # binary charset: a byte slice
        want.append((len(b[:k]), 0))
    lines.append("p -1 1 " + hexs(b"\xffabc"))  # no prefix length: the whole cell
    want.append((4, 0))
    for cell, k, kept, bad in [(b"\xffabc", 2, 2, 1),       # truncated, an invalid byte among the kept runes
                               (b"ab\xffc", 2, 2, 0),       # the invalid byte lies behind the cut
                               (b"ab\xffc", 3, 3, 1),
                               (b"\xffabc", 4, 4, 0),       # not truncated: never touched
                               (b"\xffabc", 9, 4, 0),
                               (b"\xc3\xa9\xc3\xa9\xc3\xa9", 4, 6, 0),  # 3 runes in 6 bytes: more bytes than the prefix, not more runes
                               (b"\xc3\xa9\xc3\xa9\xc3", 2, 4, 0),      # the cut-off rune behind the cut is one more (invalid) rune
                               (b"\xc3\xa9\xc3", 2, 3, 0),              # two runes (the second invalid): nothing to cut
                               (b"a\xe4\xb8b", 2, 2, 1)]:
        lines.append("p %d 1 %s" % (k, hexs(cell)))
        want.append((kept, bad))
        lines.append("p %d 0 %s" % (k, hexs(cell)))
        want.append((min(k, len(cell)), 0))
    got = dp(lines)
    assert [(int(g[0]), int(g[1])) for g in got] == want


def test_new_abi_is_declared_exported_and_the_version_stays():
    assert abi.TSQ_ABI_VERSION == 10
    lib = _lib.load()
    for name in ("tsq_rowcodec_encode", "tsq_indexkeys_encode"):
        assert name in abi.SIGNATURES and hasattr(lib, name)
    assert lib.tsq_abi_version() == 10
    assert abi.IDX_UNIQUE == 1 and abi.KNOB_ROWENC_WAVE_COPY == 45
