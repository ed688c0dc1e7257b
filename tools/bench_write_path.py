#!/usr/bin/env python3
"""The write path on device columns: tsq_rowcodec_encode (chunk rows -> stored rows) and tsq_indexkeys_encode (chunk rows -> index entries),
csrc/tsq_rowenc.hip, beside their sibling tsq_rows_encode (chunk rows -> response datums) on the same columns in the same run.

Workload: --rows rows (default 1e8) generated in HBM (tsq_gen_column):
  fixed   three BIGINT (i, uniform in [0, 1000), uniform in [0, 1e12)) + one DOUBLE in [0, 1)
  strings the same plus an 8-byte and a 200-byte string column (the bytes of generated BIGINTs; offsets uploaded)
  index   keys on (BIGINT uniform in [0, 1e12)) and on (that BIGINT, the 8-byte string), unique and non-unique
Every call asks for the size first (cap_bytes = 0), then encodes into HBM; ms = device events around the encoding call (its own size pass
included), median [min .. max] of --reps passes after one warm-up.  Bytes moved = the columns read twice (8 B per fixed-width cell; a string
cell: its offset twice, its bytes once: the size pass does not read them) + the bytes written + 8 B of row offset per row (index: two
offsets, the value and the distinct flag); the fraction is of 8 TB/s.  The yardstick is tsq_rows_encode on the same columns (the index
cases: TSQ_ENC_COMPARABLE on every column): a result slower than it by more than the extra bytes written explain is a finding.
A/B of the long-cell threshold (TSQ_KNOB_ROWENC_WAVE_COPY): the strings case and the (BIGINT, 8-byte string) index at each --thresholds value
(0 = the row's lane copies every cell).
Host leg: the CPU oracle's encoders (the C++ restatement the tests compare with) on --host-rows rows, one thread.
   python tools/bench_write_path.py [--rows 1e8] [--reps 3] [--host-rows 1e7] [--thresholds 0,8,64,256] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3


def spec(kind, col, m=0):
    s = abi.GenSpec()
    s.kind, s.table, s.col, s.seed, s.m = kind, 14, col, 77, m
    return s


def dev_col(ptr, tp, n, offsets=None):
    c = abi.Col()
    c.data, c.length, c.elem_size, c.type, c.flags, c.offsets = ptr, n, (-1 if tp == abi.BYTES else 8), tp, abi.COL_DEVICE, offsets
    return c


def _mmm(v):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))


class Bench:
    def __init__(self, ctx, n, reps):
        self.ctx, self.n, self.reps = ctx, n, reps
        self.lines, self.results = [], []

    def say(self, line, rec):
        self.lines.append(line)
        self.results.append(rec)
        print(line, flush=True)

    def timed(self, size_call, call, extra_bytes):
        """size_call() -> bytes needed; call(out, offs, cap) encodes.  Returns (ms list, bytes written)"""
        ctx = self.ctx
        need = size_call()
        out, offs = ctx.alloc(need + 64), ctx.alloc((self.n + 1) * 8 + 64)
        extra = [ctx.alloc(b + 64) for b in extra_bytes]
        ms = []
        try:
            for it in range(self.reps + 1):
                ctx.sync()
                ctx.timer_start()
                call(out, offs, need, extra)
                t = ctx.timer_stop_ms()
                if it:
                    ms.append(t)
        finally:
            for p in [out, offs] + extra:
                ctx.free(p)
        return ms, need

    def report(self, what, name, ms, written, read_bytes, aux_bytes, note=""):
        med = float(np.median(ms))
        moved = read_bytes + written + aux_bytes
        self.say("%-9s %-34s %s ms   %7.1f B/row written   %7.1f B/row moved = %.4f of 8 TB/s   %.1f Mrows/s%s" % (
            what, name, _mmm(ms), written / self.n, moved / self.n, moved / (med * HBM_BYTES_PER_MS), self.n / med / 1e3, note),
            {"call": what, "case": name, "ms": ms, "bytes_written": written, "bytes_moved": moved})
        return med

    def rows_encode(self, name, cols, read_bytes, comparable=False):
        lib, ctx, n = self.ctx.lib, self.ctx, self.n
        arr = (abi.Col * len(cols))(*cols)
        fl = (C.c_uint32 * len(cols))(*[abi.ENC_COMPARABLE if comparable else 0] * len(cols))
        m = C.c_int64(0)

        def size():
            lib.tsq_rows_encode(ctx.h, arr, len(cols), fl, n, None, 0, 0, None, C.byref(m))
            return m.value

        def call(out, offs, cap, extra):
            _lib.check(lib.tsq_rows_encode(ctx.h, arr, len(cols), fl, n, C.c_void_p(out), cap, abi.COL_DEVICE, C.c_void_p(offs), C.byref(m)), ctx.h)
        ms, w = self.timed(size, call, [])
        return self.report("rows_enc", name, ms, w, read_bytes, 8 * n)

    def rowcodec(self, name, cols, read_bytes, yard=None):
        lib, ctx, n = self.ctx.lib, self.ctx, self.n
        arr = (abi.Col * len(cols))(*cols)
        ids = (C.c_int64 * len(cols))(*range(1, len(cols) + 1))
        m = C.c_int64(0)

        def size():
            lib.tsq_rowcodec_encode(ctx.h, arr, len(cols), ids, None, n, None, 0, 0, None, C.byref(m))
            return m.value

        def call(out, offs, cap, extra):
            _lib.check(lib.tsq_rowcodec_encode(ctx.h, arr, len(cols), ids, None, n, C.c_void_p(out), cap, abi.COL_DEVICE, C.c_void_p(offs), C.byref(m)), ctx.h)
        ms, w = self.timed(size, call, [])
        return self.report("rowcodec", name, ms, w, read_bytes, 8 * n, "" if yard is None else "   %.2f x tsq_rows_encode" % (float(np.median(ms)) / yard))

    def indexkeys(self, name, cols, handles, unique, read_bytes, yard=None):
        lib, ctx, n = self.ctx.lib, self.ctx, self.n
        arr = (abi.Col * len(cols))(*cols)
        m = C.c_int64(0)
        one = np.zeros(2, np.int64)
        p1 = one.ctypes.data_as(C.c_void_p)
        fl = abi.IDX_UNIQUE if unique else 0

        def size():
            lib.tsq_indexkeys_encode(ctx.h, 41, 7, fl, arr, len(cols), None, None, C.c_void_p(handles), n, 0, None, 0, p1, None, p1, None, C.byref(m))
            return m.value

        def call(out, offs, cap, extra):
            _lib.check(lib.tsq_indexkeys_encode(ctx.h, 41, 7, fl, arr, len(cols), None, None, C.c_void_p(handles), n, abi.COL_DEVICE, C.c_void_p(out), cap,
                                                C.c_void_p(offs), C.c_void_p(extra[0]), C.c_void_p(extra[1]), C.c_void_p(extra[2]), C.byref(m)), ctx.h)
        ms, w = self.timed(size, call, [8 * n, 8 * (n + 1), n])
        vbytes = (8 if unique else 1) * n
        return self.report("indexkeys", name, ms, w, read_bytes + 16 * n, 17 * n + vbytes, "" if yard is None else "   %.2f x tsq_rows_encode" % (float(np.median(ms)) / yard))


def host_leg(b, hn):
    """the CPU oracle's encoders on hn rows of the same kinds of columns, one thread"""
    from oracle import binding as orc
    from tinysql_amd.chunk import Chunk, Column
    rng = np.random.default_rng(1)
    chk = Chunk([Column(abi.I64, np.arange(hn)), Column(abi.I64, rng.integers(0, 1000, hn)), Column(abi.I64, rng.integers(0, 10 ** 12, hn)), Column(abi.F64, rng.random(hn))])
    orc.load()
    t0 = time.perf_counter()
    raw, _ = orc.rowcodec_encode(chk, [1, 2, 3, 4])
    t1 = time.perf_counter()
    b.say("host oracle rowcodec fixed, %d rows: %.1f ms = %.2f Mrows/s, %.1f B/row, one thread" % (hn, (t1 - t0) * 1e3, hn / (t1 - t0) / 1e6, raw.size / hn),
          {"call": "host_rowcodec", "rows": hn, "ms": (t1 - t0) * 1e3})
    t0 = time.perf_counter()
    keys, _ = orc.encode_index_keys(Chunk([chk.columns[2]]), 41, 7, np.arange(hn, dtype=np.int64), np.ones(hn, np.uint8))
    t1 = time.perf_counter()
    b.say("host oracle index keys (BIGINT) non-unique, %d rows: %.1f ms = %.2f Mrows/s, %.1f B/row, one thread" % (hn, (t1 - t0) * 1e3, hn / (t1 - t0) / 1e6, keys.size / hn),
          {"call": "host_indexkeys", "rows": hn, "ms": (t1 - t0) * 1e3})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1e8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", default="1e7")
    ap.add_argument("--thresholds", default="0,8,64,256")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, hn = int(float(a.rows)), int(float(a.host_rows))
    with _lib.Context(0) as ctx:
        b = Bench(ctx, n, a.reps)
        b.lines.append("%d device-resident rows; ms = device events around the encoding call, median [min .. max] of %d passes after one warm-up" % (n, a.reps))
        print(b.lines[0], flush=True)
        ptr = [ctx.alloc(n * 8 + 64) for _ in range(5)]
        long_data = ctx.alloc(n * 200 + 64)
        offs8, offs200 = ctx.alloc((n + 1) * 8 + 64), ctx.alloc((n + 1) * 8 + 64)
        try:
            ctx.gen_column(spec(abi.GEN_SEQ, 0), n, ptr[0])
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 1, 1000), n, ptr[1])
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 2, 10 ** 12), n, ptr[2])
            ctx.gen_column(spec(abi.GEN_RAND_F64, 3), n, ptr[3])
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 4, 1000000), n, ptr[4])
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 5, 1 << 62), n * 25, long_data)
            ctx.h2d(offs8, np.arange(n + 1, dtype=np.int64) * 8)
            ctx.h2d(offs200, np.arange(n + 1, dtype=np.int64) * 200)
            fixed = [dev_col(ptr[0], abi.I64, n), dev_col(ptr[1], abi.I64, n), dev_col(ptr[2], abi.I64, n), dev_col(ptr[3], abi.F64, n)]
            s8, s200 = dev_col(ptr[4], abi.BYTES, n, offs8), dev_col(long_data, abi.BYTES, n, offs200)
            rd_fixed = 4 * 16 * n
            rd_str = rd_fixed + (16 + 8) * n + (16 + 200) * n
            y = b.rows_encode("3 BIGINT + DOUBLE", fixed, rd_fixed)
            b.rowcodec("3 BIGINT + DOUBLE", fixed, rd_fixed, y)
            y = b.rows_encode("+ 8-byte + 200-byte strings", fixed + [s8, s200], rd_str)
            b.rowcodec("+ 8-byte + 200-byte strings", fixed + [s8, s200], rd_str, y)
            y1 = b.rows_encode("(BIGINT) comparable", [fixed[2]], 16 * n, comparable=True)
            y2 = b.rows_encode("(BIGINT, 8-byte string) comparable", [fixed[2], s8], (16 + 24) * n, comparable=True)
            for unique in (False, True):
                u = "unique" if unique else "non-unique"
                b.indexkeys("(BIGINT) " + u, [fixed[2]], ptr[0], unique, 16 * n, y1)
                b.indexkeys("(BIGINT, 8-byte string) " + u, [fixed[2], s8], ptr[0], unique, (16 + 24) * n, y2)
            for thr in [int(x) for x in a.thresholds.split(",") if x != ""]:
                ctx.set_knob(abi.KNOB_ROWENC_WAVE_COPY, thr)
                b.rowcodec("strings, wave copy from %d B" % thr, fixed + [s8, s200], rd_str)
                b.rowcodec("3 BIGINT + DOUBLE + 8-byte, from %d B" % thr, fixed + [s8], rd_fixed + 24 * n)
                b.indexkeys("(BIGINT, 8-byte), wave copy from %d B" % thr, [fixed[2], s8], ptr[0], False, (16 + 24) * n)
                b.indexkeys("(BIGINT, 200-byte), wave copy from %d B" % thr, [fixed[2], s200], ptr[0], False, (16 + 216) * n)
            ctx.set_knob(abi.KNOB_ROWENC_WAVE_COPY)
        finally:
            for p in ptr + [long_data, offs8, offs200]:
                ctx.free(p)
        host_leg(b, min(hn, n))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(b.lines) + "\n")
            f.write(json.dumps(b.results) + "\n")
    print(json.dumps({"bench": "write_path", "cases": len(b.results)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
