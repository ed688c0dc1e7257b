#!/usr/bin/env python3
"""The per-row step of INSERT .. SELECT on device columns: tsq_cast_run and tsq_autoid_fill (csrc/tsq_insert.hip), alone and in front of
tsq_rowcodec_encode, in the same run.

Workload: --rows rows (default 1e8) generated in HBM (tsq_gen_column):
  cast     BIGINT uniform in [0, 2^31) -> INT, BIGINT uniform in [0, 256) -> TINYINT UNSIGNED NOT NULL, DOUBLE in [0, 1) -> DOUBLE(8,2)
           (no cell fails: the error and warning paths cost a wave nothing when its rows are fine)
  strings  the same three columns plus an 8-byte string -> VARCHAR(8) utf8mb4 and a 200-byte string -> VARCHAR(200) utf8mb4 (ASCII cells of exactly
           Flen bytes: every cell is rune-walked by the UTF-8 check and kept whole; the sizing call (cap_bytes = 0) is timed on its own line)
  autoid   tsq_autoid_fill on a BIGINT column: all NULL; 1 % explicit ids (uniform in [1, 2 * rows]), the rest NULL
  e2e      the cast of (id not named, the three columns above), tsq_autoid_fill on the id column, tsq_rowcodec_encode of the four columns
ms per call = device events around a window of --calls calls back to back (tsq_timer_*; tsq_autoid_fill works in place, so its window
runs over --calls copies of the column; the end-to-end window holds two rounds), median [min .. max] of --reps windows after one warm-up.
These are WHOLE-CALL times — the entry point's memsets, launches, read-back and synchronisation included — not kernel times.  Bytes that must move: the cast
reads 8 B per cell and writes 8 B per cell + one bit; tsq_autoid_fill reads the column and its bitmap twice (aggregate pass, apply pass)
and writes them once; a string cell: its two 8-byte offsets in and out and its bytes read once and written once (the length pass reads them a
second time for the UTF-8 walk: not counted); the encoder's bytes as tools/bench_write_path.py counts them.  The fraction is of 8 TB/s.
Host leg, one core, from the same run: tests/cast_ref.py (plain Python, the tests' yardstick) on --ref-rows rows and a vectorised numpy
restatement of the three casts on --host-rows rows.
   python tools/bench_insert_select.py [--rows 1e8] [--reps 9] [--calls 8] [--host-rows 1e7] [--ref-rows 2e5] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import table as T  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3


def spec(kind, col, m=0, start=0):
    s = abi.GenSpec()
    s.kind, s.table, s.col, s.seed, s.m, s.start = kind, 15, col, 78, m, start
    return s


def dev_col(ptr, tp, n, bitmap=None):
    c = abi.Col()
    c.data, c.null_bitmap, c.length, c.elem_size, c.type, c.flags = ptr, bitmap, n, 8, tp, abi.COL_DEVICE
    return c


def _mmm(v):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))


def timed(ctx, reps, call, before=None, calls=1):
    """ms per call: `calls` calls back to back inside one timed window (call(k), k = 0 .. calls - 1), reps windows after one warm-up"""
    ms = []
    for it in range(reps + 1):
        if before:
            before()
        ctx.sync()
        ctx.timer_start()
        for k in range(calls):
            call(k)
        t = ctx.timer_stop_ms() / calls
        if it:
            ms.append(t)
    return ms


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1e8")
    ap.add_argument("--reps", type=int, default=9)
    ap.add_argument("--calls", type=int, default=8)
    ap.add_argument("--host-rows", default="1e7")
    ap.add_argument("--ref-rows", default="2e5")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, hn, rn = int(float(a.rows)), int(float(a.host_rows)), int(float(a.ref_rows))
    lines, results = [], []

    def say(line, rec):
        lines.append(line)
        results.append(rec)
        print(line, flush=True)

    def report(what, ms, moved, note=""):
        med = float(np.median(ms))
        say("%-34s %s ms   %6.1f B/row moved = %.4f of 8 TB/s   %8.1f Mrows/s%s" % (what, _mmm(ms), moved / n, moved / (med * HBM_BYTES_PER_MS), n / med / 1e3, note),
            {"case": what, "ms": ms, "bytes_moved": moved, "rows": n})
        return med

    INT = T.ColumnInfo(abi.TP_LONG)
    TINY = T.ColumnInfo(abi.TP_TINY, Flag=T.UnsignedFlag | T.NotNullFlag)
    DBL = T.ColumnInfo(abi.TP_DOUBLE, 8, 2)
    ID = T.ColumnInfo(abi.TP_LONGLONG, Flag=T.AutoIncrementFlag | T.NotNullFlag | T.PriKeyFlag)
    stmt = T.StatementContext()
    with _lib.Context(0) as ctx:
        lib = ctx.lib
        say("%d device-resident rows; ms per call = device events around a window of %d calls (whole calls: memsets, launches, read-back, synchronisation), "
            "median [min .. max] of %d windows after one warm-up" % (n, a.calls, a.reps), {"rows": n})
        bm = (n + 7) // 8 + 64
        src = [ctx.alloc(n * 8 + 64) for _ in range(3)]
        out = [ctx.alloc(n * 8 + 64) for _ in range(4)]
        obm = [ctx.alloc(bm) for _ in range(4)]
        ids_src, ids_bm_src = ctx.alloc(n * 8 + 64), ctx.alloc(bm)
        idw = [(ctx.alloc(n * 8 + 64), ctx.alloc(bm)) for _ in range(max(a.calls - 1, 0))]  # further working copies of the id column
        try:
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 1, 1 << 31), n, src[0])
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 2, 256), n, src[1])
            ctx.gen_column(spec(abi.GEN_RAND_F64, 3), n, src[2])
            ins = (abi.Col * 3)(dev_col(src[0], abi.I64, n), dev_col(src[1], abi.I64, n), dev_col(src[2], abi.F64, n))
            # ---- the cast alone
            cast = T.Caster(ctx, [INT, TINY, DBL], [0, 1, 2], [abi.I64, abi.I64, abi.F64], stmt)
            outs = (abi.Col * 3)(dev_col(out[1], abi.I64, n, obm[1]), dev_col(out[2], abi.U64, n, obm[2]), dev_col(out[3], abi.F64, n, obm[3]))
            ms = timed(ctx, a.reps, lambda k: _lib.check(lib.tsq_cast_run(cast.h, ins, 3, n, outs, None, None), cast.h), calls=a.calls)
            report("cast  INT, TINYINT UNSIGNED, DOUBLE(8,2)", ms, 3 * (16 * n + n // 8))
            cast.close()
            # ---- ... plus an 8-byte and a 200-byte string column
            sdata = [ctx.alloc(n * 8 + 64), ctx.alloc(n * 200 + 64)]
            soffs = [ctx.alloc((n + 1) * 8 + 64) for _ in range(2)]
            odata = [ctx.alloc(n * 8 + 64), ctx.alloc(n * 200 + 64)]
            ooffs = [ctx.alloc((n + 1) * 8 + 64) for _ in range(2)]
            sbm = [ctx.alloc(bm) for _ in range(2)]
            try:
                ctx.memset(sdata[0], 0x62, n * 8)
                ctx.memset(sdata[1], 0x61, n * 200)
                ctx.h2d(soffs[0], np.arange(n + 1, dtype=np.int64) * 8)
                ctx.h2d(soffs[1], np.arange(n + 1, dtype=np.int64) * 200)

                def scol(data, offs, bitmap=None):
                    c = abi.Col()
                    c.data, c.null_bitmap, c.offsets, c.length, c.elem_size, c.type, c.flags = data, bitmap, offs, n, -1, abi.BYTES, abi.COL_DEVICE
                    return c
                ins5 = (abi.Col * 5)(ins[0], ins[1], ins[2], scol(sdata[0], soffs[0]), scol(sdata[1], soffs[1]))
                outs5 = (abi.Col * 5)(outs[0], outs[1], outs[2], scol(odata[0], ooffs[0], sbm[0]), scol(odata[1], ooffs[1], sbm[1]))
                V8, V200 = T.ColumnInfo(abi.TP_VARCHAR, 8, Charset="utf8mb4"), T.ColumnInfo(abi.TP_VARCHAR, 200, Charset="utf8mb4")
                cast = T.Caster(ctx, [INT, TINY, DBL, V8, V200], [0, 1, 2, 3, 4], [abi.I64, abi.I64, abi.F64, abi.BYTES, abi.BYTES], stmt)
                cap0, cap, need = (C.c_int64 * 5)(), (C.c_int64 * 5)(0, 0, 0, n * 8, n * 200), (C.c_int64 * 5)()

                def ask(k):
                    assert lib.tsq_cast_run(cast.h, ins5, 5, n, outs5, cap0, need) == abi.ERR_INVALID and need[4] == n * 200
                ms = timed(ctx, a.reps, ask, calls=2)
                report("strings: the sizing call alone", ms, 3 * 8 * n + 2 * 8 * n + 208 * n)
                ms = timed(ctx, a.reps, lambda k: _lib.check(lib.tsq_cast_run(cast.h, ins5, 5, n, outs5, cap, need), cast.h), calls=2)
                report("cast  + VARCHAR(8) + VARCHAR(200)", ms, 3 * (16 * n + n // 8) + 2 * (16 * n + n // 8) + 2 * 208 * n)
                cast.close()
            finally:
                for p_ in sdata + soffs + odata + ooffs + sbm:
                    ctx.free(p_)
            # ---- tsq_autoid_fill alone
            nb = C.c_int64(0)

            def fill(col):
                _lib.check(lib.tsq_autoid_fill(ctx.h, C.byref(col), n, 0, 0, (1 << 63) - 1, C.byref(nb), None, None, None), ctx.h)
            work = [(out[0], obm[0])] + idw
            idc = [dev_col(d, abi.I64, n, b) for d, b in work]
            for name, explicit in (("all NULL", False), ("1 % explicit ids", True)):
                if explicit:  # made on the host in pieces
                    rng = np.random.default_rng(4)
                    piece = 1 << 24
                    for lo in range(0, n, piece):
                        m = min(piece, n - lo)
                        keep = rng.random(m) < 0.01
                        v = np.where(keep, rng.integers(1, 2 * n + 1, m), 0).astype(np.int64)
                        ctx.h2d(ids_src + 8 * lo, v)
                        ctx.h2d(ids_bm_src + lo // 8, np.packbits(keep, bitorder="little"))
                else:
                    ctx.memset(ids_src, 0, n * 8)
                    ctx.memset(ids_bm_src, 0, (n + 7) // 8)

                def reset():
                    for d, b in work:
                        _lib.check(lib.tsq_copy_d2d(ctx.h, C.c_void_p(d), C.c_void_p(ids_src), n * 8), ctx.h)
                        _lib.check(lib.tsq_copy_d2d(ctx.h, C.c_void_p(b), C.c_void_p(ids_bm_src), (n + 7) // 8), ctx.h)
                ms = timed(ctx, a.reps, lambda k: fill(idc[k]), before=reset, calls=len(work))
                report("autoid " + name, ms, 3 * (8 * n + n // 8), "   new base %d" % nb.value)
            # ---- cast + auto ids + stored rows
            cast = T.Caster(ctx, [ID, INT, TINY, DBL], [-1, 0, 1, 2], [abi.I64, abi.I64, abi.F64], stmt)
            outs4 = (abi.Col * 4)(dev_col(out[0], abi.I64, n, obm[0]), dev_col(out[1], abi.I64, n, obm[1]), dev_col(out[2], abi.U64, n, obm[2]), dev_col(out[3], abi.F64, n, obm[3]))
            cids = (C.c_int64 * 4)(1, 2, 3, 4)
            need = C.c_int64(0)
            _lib.check(lib.tsq_cast_run(cast.h, ins, 3, n, outs4, None, None), cast.h)
            fill(outs4[0])
            lib.tsq_rowcodec_encode(ctx.h, outs4, 4, cids, None, n, None, 0, 0, None, C.byref(need))
            enc, enc_offs = ctx.alloc(need.value + 64), ctx.alloc((n + 1) * 8 + 64)

            def e2e(k):
                _lib.check(lib.tsq_cast_run(cast.h, ins, 3, n, outs4, None, None), cast.h)
                fill(outs4[0])
                _lib.check(lib.tsq_rowcodec_encode(ctx.h, outs4, 4, cids, None, n, C.c_void_p(enc), need.value, abi.COL_DEVICE, C.c_void_p(enc_offs), C.byref(need)), ctx.h)
            try:
                ms = timed(ctx, a.reps, e2e, calls=2)
            finally:
                ctx.free(enc)
                ctx.free(enc_offs)
            moved = (3 * 8 * n + 4 * (8 * n + n // 8)) + 3 * (8 * n + n // 8) + (4 * 16 * n + need.value + 8 * n)
            report("cast + auto ids + tsq_rowcodec_encode", ms, moved, "   %.1f B/row stored" % (need.value / n))
            cast.close()
        finally:
            for p in src + out + obm + [ids_src, ids_bm_src] + [x for pair in idw for x in pair]:
                ctx.free(p)
    # ---- host leg: one core
    from tests import cast_ref as R
    rng = np.random.default_rng(1)
    ha, hb, hc = rng.integers(0, 1 << 31, hn), rng.integers(0, 256, hn), rng.random(hn)
    t0 = time.perf_counter()
    ra = np.clip(ha, -(1 << 31), (1 << 31) - 1)
    rb = np.clip(hb, 0, 255).astype(np.uint64)
    tmp = hc * 100.0
    rc = np.clip(np.where(np.abs(tmp) < 0.5, 0.0, np.trunc(tmp + np.copysign(0.5, tmp))) / 100.0, -999999.99, 999999.99)
    bad = int((ra != ha).sum() + (rb != hb).sum() + (np.abs(rc) == 999999.99).sum())
    t1 = time.perf_counter()
    say("host numpy restatement of the three casts, %d rows: %.1f ms = %.2f Mrows/s, one core (%d cells clipped)" % (hn, (t1 - t0) * 1e3, hn / (t1 - t0) / 1e6, bad),
        {"case": "host_numpy", "rows": hn, "ms": (t1 - t0) * 1e3})
    fts = [R.FieldType(abi.TP_LONG), R.FieldType(abi.TP_TINY, unsigned=True, not_null=True), R.FieldType(abi.TP_DOUBLE, 8, 2)]
    rows = [[int(ha[i]), int(hb[i]), float(hc[i])] for i in range(rn)]
    t0 = time.perf_counter()
    R.cast_rows(abi.CAST_IN_INSERT, rows, [abi.I64, abi.I64, abi.F64], fts, [0, 1, 2])
    t1 = time.perf_counter()
    say("tests/cast_ref.py (plain Python) on the same three casts, %d rows: %.1f ms = %.3f Mrows/s, one core" % (rn, (t1 - t0) * 1e3, rn / (t1 - t0) / 1e6),
        {"case": "host_cast_ref", "rows": rn, "ms": (t1 - t0) * 1e3})
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
