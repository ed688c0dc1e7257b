"""CPU: the string arm of the filter's toBool.  tsq_str_to_int (csrc/tsq_device.h, the source the interpreter, the JIT and this
g++ build share) against the reference's own vectors (tests/golden/strtoint_cases.json, from types/convert_test.go) and against the
Python restatement of types.StrToInt (tests/strtoint_ref.py) on fuzzed strings; str_ctx validation."""
import ctypes as C
import json
import os
import subprocess

import numpy as np
import pytest

from tests import strtoint_ref as R

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))

SHIM = r"""
#include "%s"
extern "C" uint32_t s2i(const uint8_t* s, uint32_t n, uint32_t ctx, int64_t* v) { return tsq_str_to_int(s, n, ctx, v); }
extern "C" void s2i_batch(const uint8_t* data, const int64_t* offs, int64_t rows, uint32_t ctx, int64_t* v, uint32_t* f) {
    for (int64_t i = 0; i < rows; i++) f[i] = tsq_str_to_int(data + offs[i], (uint32_t)(offs[i + 1] - offs[i]), ctx, &v[i]);
}
extern "C" int32_t validate_str_ctx(int32_t ctx, int32_t result_bytes) {
    tsq_expr_prog p;
    memset(&p, 0, sizeof p);
    p.n_ops = 1;
    p.ops[0].opcode = result_bytes ? TSQ_OP_COL_STR : TSQ_OP_COL_INT;
    p.result_type = result_bytes ? TSQ_BYTES : TSQ_I64;
    p.str_ctx = ctx;
    const char* why = "";
    return tsq_validate_prog(p, 1, &why);
}
"""


@pytest.fixture(scope="module")
def lib(tmp_path_factory):
    d = tmp_path_factory.mktemp("s2i")
    src = d / "s2i.cpp"
    src.write_text(SHIM % os.path.join(ROOT, "tinysql_amd", "csrc", "tsq_device.h"))
    so = d / "s2i.so"
    subprocess.run(["g++", "-O2", "-std=c++17", "-fPIC", "-shared", "-Wall", "-Wno-unused-function", "-Wno-unknown-pragmas", "-o", str(so), str(src)], check=True)
    lib = C.CDLL(str(so))
    lib.s2i.restype = C.c_uint32
    lib.s2i.argtypes = [C.c_char_p, C.c_uint32, C.c_uint32, C.POINTER(C.c_int64)]
    lib.s2i_batch.restype = None
    lib.s2i_batch.argtypes = [C.c_void_p, C.c_void_p, C.c_int64, C.c_uint32, C.c_void_p, C.c_void_p]
    lib.validate_str_ctx.restype = C.c_int32
    return lib


def s2i(lib, b, ctx):
    v = C.c_int64()
    f = lib.s2i(b, len(b), ctx, C.byref(v))
    return v.value, f


def test_reference_vectors(lib):
    cases = json.load(open(os.path.join(ROOT, "tests", "golden", "strtoint_cases.json")))["cases"]
    assert len(cases) > 50
    for c in cases:
        b = c["s"].encode()
        want = (c["value"], c["flags"])
        assert R.str_to_int(b, c["str_ctx"]) == want, ("python", c)
        assert s2i(lib, b, c["str_ctx"]) == want, ("device", c)


HAND = [
    b"", b" ", b"0", b"-0", b"+", b"-", b"+-1", b"--.5", b"+-.5", b"-+.6", b"1+2", b"1-5e-2", b"1-9.9", b".+5e1", b"1+.5",
    b"9223372036854775807", b"9223372036854775808", b"-9223372036854775808", b"-9223372036854775809", b"18446744073709551615",
    b"18446744073709551616x", b"9223372036854775808x", b"99999999999999999999e99999999999999999999", b"1e9223372036854775808",
    b"1e-9223372036854775808", b"12e9223372036854775807", b"-5e-1", b"5e-1", b"-5e-2", b"+999.9999e2", b"0.49", b"-0.5", b"9.5",
    b"99.99e1", b"1.5x", b"1.5e30", b"125e342x", b"1e21", b"1e20", b"0.000000000000000000000000001e27", b"\xc2\xa0 12 \xe3\x80\x80",
    b"\xe2\x80\x8b1", b"1\xc2", b"\xc2 1", b"\x1c1", b"\v\f\r\n\t7\t", b"1\x85", b"\xc2\x851\xe2\x81\x9f", b"\xed\xa0\x80", b"0" * 5000 + b"1.5",
    b"1" + b"9" * 3000 + b".9", b"00000000000000000000000000012", b"0x10", b"1E2", b"1e+2", b"1e", b"1e+", b".", b".e1", b"1.e1",
]


@pytest.mark.parametrize("mode", R.ALL_CTX)
def test_hand_cases_agree(lib, mode):
    ctx = mode
    for b in HAND:
        assert s2i(lib, b, ctx) == R.str_to_int(b, ctx), (b[:40], ctx)


SPACES = [b" ", b"\t", b"\n", b"\v", b"\f", b"\r", b"\xc2\x85", b"\xc2\xa0", b"\xe1\x9a\x80", b"\xe2\x80\x80", b"\xe2\x80\x8a", b"\xe2\x80\xa8",
          b"\xe2\x80\xa9", b"\xe2\x80\xaf", b"\xe2\x81\x9f", b"\xe3\x80\x80"]
NOT_SPACES = [b"\xc2", b"\xe2\x80", b"\xe2\x80\x8b", b"\xff", b"\x80", b"\x1c", b"\xc2\x86", b"\xe3\x80"]
JUNK = [b"x", b"e", b"E", b".", b"+", b"-", b"..", b"e5", b"a1", b" 1", b"\x00", b"\xc3\xa9", b"1", b"9", b"5"]


def fuzz_strings(seed, n):
    rng = np.random.default_rng(seed)
    out = []
    r = rng.integers(0, 1 << 30, size=(n, 16))
    for i in range(n):
        x = r[i]
        parts = []
        for k in range(x[0] % 3):
            parts.append(SPACES[x[1 + k] % len(SPACES)] if x[4] % 5 else NOT_SPACES[x[1 + k] % len(NOT_SPACES)])
        if x[5] % 3 == 0:
            parts.append(b"+-"[x[6] % 2: x[6] % 2 + 1])
            if x[6] % 7 == 0:
                parts.append(b"+-"[x[7] % 2: x[7] % 2 + 1])
        nd = x[8] % 26
        digs = bytes(48 + int(d) for d in rng.integers(0, 10, nd)) if x[9] % 4 else b"9" * nd
        parts.append(digs)
        if x[10] % 3 == 0:
            parts.append(b".")
            parts.append(bytes(48 + int(d) for d in rng.integers(0, 10, x[11] % 12)) if x[9] % 5 else b"9" * (x[11] % 12))
        if x[12] % 4 == 0:
            parts.append(b"eE"[x[13] % 2: x[13] % 2 + 1])
            if x[13] % 3:
                parts.append(b"+-"[x[14] % 2: x[14] % 2 + 1])
            k = x[14] % 6
            parts.append([b"0", b"1", b"5", b"21", b"-22", b"9223372036854775807", b"9223372036854775808", b"00000000000000000000019"][(x[15] + k) % 8]
                         if x[15] % 3 == 0 else bytes(48 + int(d) for d in rng.integers(0, 10, 1 + k)))
        if x[2] % 4 == 0:
            parts.append(JUNK[x[3] % len(JUNK)])
        for k in range(x[7] % 3):
            parts.append(SPACES[x[2 + k] % len(SPACES)] if x[13] % 6 else NOT_SPACES[x[2 + k] % len(NOT_SPACES)])
        out.append(b"".join(parts))
    return out


@pytest.mark.parametrize("mode", [R.CTX_SELECT, R.CTX_DELETE, R.CTX_INSERT, R.CTX_OTHER_LOOSE, R.CTX_IGNORE])
def test_fuzz_agrees_with_the_python_restatement(lib, mode):
    ctx = mode
    n = 200_000
    strs = fuzz_strings(1000 + ctx, n)
    offs = np.zeros(n + 1, np.int64)
    offs[1:] = np.cumsum([len(s) for s in strs])
    data = np.frombuffer(b"".join(strs) + b"\0", np.uint8)
    v = np.zeros(n, np.int64)
    f = np.zeros(n, np.uint32)
    lib.s2i_batch(data.ctypes.data, offs.ctypes.data, n, ctx, v.ctypes.data, f.ctypes.data)
    seen = set()
    for i, s in enumerate(strs):
        want = R.str_to_int(s, ctx)
        assert (int(v[i]), int(f[i])) == want, (s, ctx, want, (int(v[i]), int(f[i])))
        seen.add(want[1])
    # the fuzz reaches every flag the mode can produce
    assert any(x & R.TRUNC_WARN for x in seen) or ctx & (R.TRUNCATE_ERROR | R.IGNORE_TRUNCATE)
    assert any(x & R.ERR_OVF for x in seen)
    if ctx & R.NOT_STRICT:
        assert any(x & R.OVF_WARN for x in seen)
    if ctx & R.TRUNCATE_ERROR and not ctx & R.IGNORE_TRUNCATE:
        assert any(x & R.ERR_TRUNC for x in seen)


def test_str_ctx_unknown_bit_is_invalid(lib):
    from tinysql_amd import _abi as abi
    for rb in (0, 1):
        for ctx in range(16):
            assert lib.validate_str_ctx(ctx, rb) == abi.OK
        for ctx in (16, 32, 1 << 30, -1):
            assert lib.validate_str_ctx(ctx, rb) == abi.ERR_INVALID
