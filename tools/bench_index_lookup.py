#!/usr/bin/env python3
"""IndexLookUp on a device-resident table: tsq_lookup_task + tsq_rows_gather + tsq_rowcodec_decode (csrc/tsq_lookup.hip) per task,
beside (a) the same with TSQ_KNOB_LOOKUP_STRIDE = 0 (plain lower bound over the whole table) and (b) what a caller had to do before:
decode the WHOLE table (tsq_rowcodec_decode, the storage side of tableScanExec) and hash-join it against the task's handles
(GpuHashJoinExec), per task — in the same process, on the same rows, row counts compared.

Workload: --rows rows (default 1e8) in HBM, handle = 3 i, stored rows (rowcodec v2) of three BIGINT + one DOUBLE, built on the device
with tsq_rowcodec_encode; a second table (--rows2) adds an 8-byte and a 200-byte string column.  Tasks of --tasks handles (2^14, 2^17,
2^20, 2^22): uniform = random rows of the whole table, clustered = random rows of a window of 4 x the task's size; hit 100 % = handles of
the table, 50 % = every second one moved to 3 i + 1 (not in the table); handles arrive in random order (an index order unrelated to the
handle).  Phases, each a host clock around a call that ends in a device synchronise, median [min .. max] of --reps after one warm-up:
  keep   tsq_lookup_task(keep_order = 1): search + compaction, task order
  sorted the same over handles that are already ascending: what the search costs behind the sort
  nokeep tsq_lookup_task(keep_order = 0): radix sort of the handles + search + compaction   (sort ~ nokeep - sorted)
  gather tsq_rows_gather of the found rows (size query + copy), decode tsq_rowcodec_decode of the gathered rows
Algorithmic bytes of the gather, computed here: per found row 8 (row index) + 16 (offset pair) + 2 x row bytes + 8 (offset out); the
share is of 8 TB/s.  The search has no meaningful byte count (it is latency: dependent reads), only handles per microsecond.
   python tools/bench_index_lookup.py [--rows 1e8] [--rows2 1e8] [--reps 5] [--out profiles/index_lookup_ab.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import coprocessor as cop  # noqa: E402
from tinysql_amd import gpu_pipeline as P  # noqa: E402
from tinysql_amd import rowcodec as RC  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3
LINES = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def mmm(v):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(v)), min(v), max(v))


def dev_col(data, tp, n, offsets=None):
    c = abi.Col()
    c.data, c.length, c.elem_size, c.type, c.flags, c.offsets = data, n, (-1 if tp == abi.BYTES else 8), tp, abi.COL_DEVICE, offsets
    return c


class Table:
    """n stored rows in HBM: handle = 3 i; a = i, b = 7 i mod 1000003, c = i >> 2, d = i / 2 [, s8 = 8 bytes, s200 = 200 bytes]"""

    def __init__(self, ctx, n, strings):
        self.ctx, self.n, self.strings = ctx, n, strings
        lib = ctx.lib
        self.types = [abi.I64, abi.I64, abi.I64, abi.F64] + ([abi.BYTES, abi.BYTES] if strings else [])
        cols = [ctx.alloc(n * 8 + 64) for _ in range(4)]
        self.handles = ctx.alloc(n * 8 + 64)
        step = 1 << 24
        for lo in range(0, n, step):
            i = np.arange(lo, min(n, lo + step), dtype=np.int64)
            for k, arr in enumerate([i, (i * 7) % 1000003, i >> 2, i * 0.5]):
                ctx.h2d(cols[k] + lo * 8, np.ascontiguousarray(arr))
            ctx.h2d(self.handles + lo * 8, i * 3)
        views = [dev_col(cols[k], self.types[k], n) for k in range(4)]
        extra = []
        if strings:
            rng = np.random.default_rng(1)
            for width in (8, 200):
                block_rows = min(n, 1 << 20)
                block = rng.integers(32, 127, block_rows * width, dtype=np.uint8)
                data, offs = ctx.alloc(n * width + 64), ctx.alloc((n + 1) * 8 + 64)
                ctx.h2d(data, block)
                for lo in range(block_rows, n, block_rows):  # the same block of cells again and again: the bytes do not matter here
                    cnt = min(block_rows, n - lo)
                    _lib.check(lib.tsq_copy_d2d(ctx.h, C.c_void_p(data + lo * width), C.c_void_p(data), cnt * width), ctx.h)
                for lo in range(0, n + 1, step):
                    ctx.h2d(offs + lo * 8, np.arange(lo, min(n + 1, lo + step), dtype=np.int64) * width)
                views.append(dev_col(data, abi.BYTES, n, offs))
                extra += [data, offs]
        nc = len(views)
        ca = (abi.Col * nc)(*views)
        ids = (C.c_int64 * nc)(*range(1, nc + 1))
        need = C.c_int64(0)
        st = lib.tsq_rowcodec_encode(ctx.h, ca, nc, ids, None, n, None, 0, abi.COL_DEVICE, None, C.byref(need))
        if st not in (abi.OK, abi.ERR_INVALID):
            _lib.check(st, ctx.h)
        self.n_bytes = need.value
        self.values, self.offsets = ctx.alloc(need.value + 64), ctx.alloc((n + 1) * 8 + 64)
        _lib.check(lib.tsq_rowcodec_encode(ctx.h, ca, nc, ids, None, n, C.c_void_p(self.values), need.value, abi.COL_DEVICE, C.c_void_p(self.offsets), C.byref(need)), ctx.h)
        for p in cols + extra:
            ctx.free(p)
        self.infos = [RC.ColInfo(1, RC.TypeLonglong), RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(3, RC.TypeLonglong), RC.ColInfo(4, RC.TypeDouble)]
        if strings:
            self.infos += [RC.ColInfo(5, RC.TypeVarchar), RC.ColInfo(6, RC.TypeVarchar)]
        self.rc = (abi.RowcodecCol * len(self.infos))()
        for k, c in enumerate(self.infos):
            self.rc[k].col_id, self.rc[k].type = c.ID, c.tsq_type()

    def lookup(self, stride=None):
        ctx = self.ctx
        ctx.set_knob(abi.KNOB_LOOKUP_STRIDE, abi.KNOB_DEFAULT if stride is None else stride)
        h = C.c_void_p()
        t0 = time.perf_counter()
        _lib.check(ctx.lib.tsq_lookup_create(ctx.h, C.c_void_p(self.handles), self.n, abi.COL_DEVICE, C.byref(h)), ctx.h)
        ms = (time.perf_counter() - t0) * 1e3
        ctx.set_knob(abi.KNOB_LOOKUP_STRIDE)
        return h, ms

    def free(self):
        for p in (self.handles, self.values, self.offsets):
            self.ctx.free(p)


def make_task(rng, n, size, clustered, hit50):
    if clustered:
        w = min(n, 4 * size)
        lo = int(rng.integers(0, n - w + 1))
        rows = lo + rng.integers(0, w, size)
    else:
        rows = rng.integers(0, n, size)
    h = rows.astype(np.int64) * 3
    if hit50:
        h[1::2] += 1
    return h


class Task:
    """one task's device buffers"""

    def __init__(self, ctx, handles):
        self.ctx, self.n = ctx, handles.size
        n = self.n
        self.h, self.hs = ctx.alloc(n * 8 + 64), ctx.alloc(n * 8 + 64)
        ctx.h2d(self.h, handles)
        ctx.h2d(self.hs, np.sort(handles))
        self.rows, self.hout, self.goffs = ctx.alloc(n * 8 + 64), ctx.alloc(n * 8 + 64), ctx.alloc((n + 1) * 8 + 64)

    def free(self):
        for p in (self.h, self.hs, self.rows, self.hout, self.goffs):
            self.ctx.free(p)


def timed(ctx, fn, reps):
    fn()  # warm-up
    ctx.sync()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        ctx.sync()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def lookup_call(ctx, lk, task, src, keep):
    nf = C.c_int64(0)
    _lib.check(ctx.lib.tsq_lookup_task(lk, C.c_void_p(src), task.n, abi.COL_DEVICE, keep, C.c_void_p(task.rows), C.c_void_p(task.hout), C.byref(nf)), lk)
    return nf.value


def gather_call(ctx, table, task, m, gvals, cap):
    need = C.c_int64(0)
    args = (ctx.h, C.c_void_p(table.values), table.n_bytes, C.c_void_p(table.offsets), table.n, C.c_void_p(task.rows), m)
    st = ctx.lib.tsq_rows_gather(*args, None, 0, None, C.byref(need))
    if st not in (abi.OK, abi.ERR_INVALID):
        _lib.check(st, ctx.h)
    assert need.value <= cap
    _lib.check(ctx.lib.tsq_rows_gather(*args, C.c_void_p(gvals), need.value, C.c_void_p(task.goffs), C.byref(need)), ctx.h)
    return need.value


class Decoded:
    def __init__(self, ctx, table, cap_rows, cap_bytes):
        self.cols = [P.DeviceColumn(ctx, t, cap_rows, cap_bytes=cap_bytes if t == abi.BYTES else 0) for t in table.types]

    def free(self):
        for c in self.cols:
            c.free()


def decode_call(ctx, table, task, m, gvals, nbytes, dec):
    oc = (abi.Col * len(dec.cols))(*[c.col(m) for c in dec.cols])
    got = C.c_int64(0)
    _lib.check(ctx.lib.tsq_rowcodec_decode(ctx.h, C.c_void_p(gvals), nbytes, C.c_void_p(task.goffs), C.c_void_p(task.hout), m, abi.COL_DEVICE, len(table.infos), table.rc, oc,
                                           C.byref(got)), ctx.h)
    return got.value


# ---------------------------------------------------------------- yardstick (b): whole-table decode + hash join per task
class _Sized:
    def __init__(self, p, size):
        self.p, self.size = p, size


class ResidentScan(cop.tableScanExec):
    """tableScanExec over KV pairs that already are in HBM (no upload in Open): the decode of the whole table, batch by batch"""

    def __init__(self, ctx, table, batch_rows):
        infos = table.infos + [RC.ColInfo(-1, RC.TypeLonglong, IsPKHandle=True)]
        P.GpuExecutor.__init__(self, ctx, [c.tsq_type() for c in infos])
        self.columns, self.n, self.batch = infos, table.n, (batch_rows + 7) & ~7
        self.raw_vals = _Sized(None, table.n_bytes)
        self.dv, self.do, self.dh = _Sized(table.values, 0), _Sized(table.offsets, 0), table.handles
        self.rc = (abi.RowcodecCol * len(infos))()
        for i, c in enumerate(infos):
            self.rc[i].col_id, self.rc[i].type, self.rc[i].flags = c.ID, c.tsq_type(), abi.RC_HANDLE if c.IsPKHandle else 0
        self.out, self.pos, self.count = None, 0, 0
        self.var_bytes = int(table.n_bytes / table.n * self.batch * 1.1) + 4096

    def Open(self):
        if self.out is None:
            self.out = self._buffers(self.batch, var_bytes=[self.var_bytes] * len(self.types))
        self.pos = self.count = 0

    def Close(self):
        pass

    def release(self):
        if self.out:
            for c in self.out:
                c.free()
        self.out = None


class _Handles(P.GpuExecutor):
    def __init__(self, ctx, ptr, n):
        super().__init__(ctx, [abi.I64])
        self.chunk, self.done = P.DeviceChunk([P.DeviceColumn(ctx, abi.I64, n, data=ptr)], n), False

    def Open(self):
        self.done = False

    def Next(self):
        if self.done:
            return P.EOS
        self.done = True
        return self.chunk


def scan_join_rows(ctx, scan, task):
    """rows of (whole-table scan) JOIN (task handles) on the handle; returns the row count"""
    j = P.GpuHashJoinExec(ctx, scan, _Handles(ctx, task.h, task.n), [len(scan.Schema()) - 1], [0], abi.JOIN_INNER, 1)
    j.Open()
    rows = 0
    try:
        while True:
            chk = j.Next()
            if chk.NumRows() == 0:
                return rows
            rows += chk.NumRows()
    finally:
        j.Close()


# ---------------------------------------------------------------- sections
def section_lookup(ctx, table, sizes, strides, reps, rng):
    say("== handle lookup, %d table rows: ms per task, median [min .. max] of %d; stride = TSQ_KNOB_LOOKUP_STRIDE (0: plain lower bound)" % (table.n, reps))
    say("%-7s %-9s %-5s %8s | %-30s | %-30s | %-30s | %9s" % ("stride", "dist", "hit", "task", "keep (task order)", "sorted input", "nokeep (sort + search)", "keep h/us"))
    tasks = {}
    for size in sizes:
        for clustered in (False, True):
            for hit50 in (False, True):
                tasks[(size, clustered, hit50)] = Task(ctx, make_task(rng, table.n, size, clustered, hit50))
    best = {}
    try:
        for stride in strides:
            lk, create_ms = table.lookup(stride)
            say("stride %s: tsq_lookup_create %.2f ms" % ("default" if stride is None else stride, create_ms))
            try:
                for (size, clustered, hit50), t in tasks.items():
                    keep = timed(ctx, lambda: lookup_call(ctx, lk, t, t.h, 1), reps)
                    srt = timed(ctx, lambda: lookup_call(ctx, lk, t, t.hs, 1), reps)
                    nokeep = timed(ctx, lambda: lookup_call(ctx, lk, t, t.h, 0), reps)
                    found = lookup_call(ctx, lk, t, t.h, 0)
                    want = size if not hit50 else size - size // 2
                    assert found == want, (found, want)
                    say("%-7s %-9s %-5s %8d | %s | %s | %s | %9.1f" % ("dflt" if stride is None else stride, "clustered" if clustered else "uniform", "50%" if hit50 else "100%",
                                                                       size, mmm(keep), mmm(srt), mmm(nokeep), size / (np.median(keep) * 1e3)))
                    best.setdefault((size, clustered, hit50), {})[stride] = (float(np.median(keep)), min(keep), max(keep), float(np.median(nokeep)), min(nokeep), max(nokeep))
            finally:
                ctx.lib.tsq_lookup_destroy(lk)
    finally:
        for t in tasks.values():
            t.free()
    say("-- per stride: sum over all tasks above of the medians (keep, nokeep), and the largest (max - min) / median of one configuration")
    for stride in strides:
        k = sum(v[stride][0] for v in best.values())
        nk = sum(v[stride][3] for v in best.values())
        spread = max(max((v[stride][2] - v[stride][1]) / v[stride][0], (v[stride][5] - v[stride][4]) / v[stride][3]) for v in best.values())
        say("stride %-7s keep %9.3f ms  nokeep %9.3f ms  worst spread %5.1f %%" % ("dflt" if stride is None else stride, k, nk, 100 * spread))
    say()


def section_gather(ctx, table, sizes, reps, rng, label, wave_copies):
    say("== gather + decode, %s (%d rows, %.1f stored bytes per row): ms, median [min .. max] of %d; wc = TSQ_KNOB_GATHER_WAVE_COPY" % (label, table.n, table.n_bytes / table.n, reps))
    say("%-9s %-6s %8s %8s | %-30s %7s %6s | %-30s" % ("dist", "wc", "task", "found", "gather", "GB", "% 8TB/s", "decode"))
    lk, _ = table.lookup(None)
    try:
        for size in sizes:
            for clustered in (False, True):
                for keep in (1, 0):
                    t = Task(ctx, make_task(rng, table.n, size, clustered, False))
                    m = lookup_call(ctx, lk, t, t.h, keep)
                    cap = int(table.n_bytes / table.n * m * 1.5) + 4096
                    gvals = ctx.alloc(cap + 64)
                    dec = Decoded(ctx, table, m, cap)
                    try:
                        for wc in wave_copies:
                            ctx.set_knob(abi.KNOB_GATHER_WAVE_COPY, abi.KNOB_DEFAULT if wc is None else wc)
                            nbytes = gather_call(ctx, table, t, m, gvals, cap)
                            g = timed(ctx, lambda: gather_call(ctx, table, t, m, gvals, cap), reps)
                            moved = m * 32 + 2 * nbytes
                            line = "%-9s %-6s %8d %8d | %s %7.3f %6.1f |" % (("clustered" if clustered else "uniform") + ("/k" if keep else "/s"), "dflt" if wc is None else wc, size, m,
                                                                             mmm(g), moved / 1e9, 100 * moved / (np.median(g) * HBM_BYTES_PER_MS))
                            if wc is None:
                                d = timed(ctx, lambda: decode_call(ctx, table, t, m, gvals, nbytes, dec), reps)
                                assert decode_call(ctx, table, t, m, gvals, nbytes, dec) == m
                                line += " " + mmm(d)
                            say(line)
                        ctx.set_knob(abi.KNOB_GATHER_WAVE_COPY)
                    finally:
                        dec.free()
                        ctx.free(gvals)
                        t.free()
    finally:
        ctx.lib.tsq_lookup_destroy(lk)
    say("(dist /k: rows in task order, keep_order = 1; /s: ascending handles, keep_order = 0)")
    say()


def section_scan_join(ctx, table, sizes, reps, rng):
    say("== yardstick (b): decode of the whole table + GpuHashJoinExec against the task's handles, per task, beside lookup + gather + decode (uniform, 100 %% hit): ms, median [min .. max] of %d" % reps)
    say("%8s | %-30s | %-30s | rows" % ("task", "scan + hash join", "lookup + gather + decode"))
    lk, _ = table.lookup(None)
    scan = ResidentScan(ctx, table, 1 << 24)
    try:
        for size in sizes:
            t = Task(ctx, make_task(rng, table.n, size, False, False))
            cap = int(table.n_bytes / table.n * size * 1.5) + 4096
            gvals = ctx.alloc(cap + 64)
            dec = Decoded(ctx, table, size, cap)
            try:
                def ours():
                    m = lookup_call(ctx, lk, t, t.h, 0)
                    nb = gather_call(ctx, table, t, m, gvals, cap)
                    return decode_call(ctx, table, t, m, gvals, nb, dec)
                rows_b = scan_join_rows(ctx, scan, t)
                rows_a = ours()
                b = timed(ctx, lambda: scan_join_rows(ctx, scan, t), reps)
                a = timed(ctx, ours, reps)
                say("%8d | %s | %s | %d %s %d" % (size, mmm(b), mmm(a), rows_b, "==" if rows_a == rows_b else "!=", rows_a))
            finally:
                dec.free()
                ctx.free(gvals)
                t.free()
    finally:
        scan.release()
        ctx.lib.tsq_lookup_destroy(lk)
    say("(a task's handles are drawn with replacement: a handle drawn twice gives two rows on both sides)")
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=float, default=1e8)
    ap.add_argument("--rows2", type=float, default=1e8)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--tasks", default="16384,131072,1048576,4194304")
    ap.add_argument("--strides", default="0,2,4,6,8,10")
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    sizes = [int(float(x)) for x in a.tasks.split(",")]
    strides = [int(x) for x in a.strides.split(",")]
    rng = np.random.default_rng(46)
    with _lib.Context(0) as ctx:
        say("tools/bench_index_lookup.py --rows %g --rows2 %g --reps %d --tasks %s --strides %s" % (a.rows, a.rows2, a.reps, a.tasks, a.strides))
        t0 = time.perf_counter()
        table = Table(ctx, int(a.rows), False)
        say("table 1 built in %.1f s: %d rows, %.2f GB of stored rows" % (time.perf_counter() - t0, table.n, table.n_bytes / 1e9))
        say()
        try:
            section_lookup(ctx, table, sizes, strides, a.reps, rng)
            section_gather(ctx, table, sizes, a.reps, rng, "table 1: three BIGINT + one DOUBLE", [None, 0, 8, 64, 256])
            section_scan_join(ctx, table, sizes, max(2, a.reps // 2), rng)
        finally:
            table.free()
        if a.rows2 > 0:
            t0 = time.perf_counter()
            table2 = Table(ctx, int(a.rows2), True)
            say("table 2 built in %.1f s: %d rows, %.2f GB of stored rows" % (time.perf_counter() - t0, table2.n, table2.n_bytes / 1e9))
            say()
            try:
                section_gather(ctx, table2, sizes, a.reps, rng, "table 2: + an 8-byte and a 200-byte string column", [None, 0, 8, 64, 256])
            finally:
                table2.free()
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
