#!/usr/bin/env python3
"""ANALYZE TABLE on device columns: the column collector (tsq_analyze_*) and the sorted histogram (tsq_sorted_hist_*), csrc/tsq_analyze.hip.

Workload: --rows rows (default 1e8) generated in HBM (tsq_gen_column):
  uniq   BIGINT, v = i                      (a primary key: every value once)
  k1000  BIGINT uniform in [0, 1000)
  k3     BIGINT uniform in [0, 3)           (low NDV: whole waves meet in three CM counters per sketch row)
  real   DOUBLE uniform in [0, 1)
  str    8-byte strings: the bytes of a BIGINT uniform in [0, 1e6) (offsets uploaded)
Collector: CM 5 x 2048, FM 10000, 10000 samples, TSQ_AN_WRAP_BYTES — per column, the four columns in one handle, and uniq / k1000 / k3 without a CM
sketch (the cost of the LDS atomics, also where a whole wave meets one counter).  ms = device events around the pushes' kernels (tsq_analyze_stats) and the
wall time of push + finish; fraction of 8 TB/s over the column bytes read (8 B per fixed cell, 16 B per string cell: bytes + an offset).
Sorted histogram of uniq, 256 buckets: scan (run heads + positions) and walk (one workgroup) timed separately (tsq_sorted_hist_stats).
Host leg: the same per-cell arithmetic (datum bytes, murmur3 tail path, CM counters, FM set) in numpy on --host-rows rows of uniq and
k1000, one process — rows per second beside the GPU's.
   python tools/bench_analyze.py [--rows 1e8] [--reps 3] [--host-rows 1e7] [--out FILE]"""
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
from tinysql_amd.statistics import AnalyzeCollector, SortedBuilder  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3
U = np.uint64


def spec(kind, col, m=0):
    s = abi.GenSpec()
    s.kind, s.table, s.col, s.seed, s.m = kind, 12, col, 99, m
    return s


def dev_col(ptr, tp, n, offsets=None):
    c = abi.Col()
    c.data, c.length, c.elem_size, c.type, c.flags, c.offsets = ptr, n, (-1 if tp == abi.BYTES else 8), tp, abi.COL_DEVICE, offsets
    return c


class Cols:
    def __init__(self, cols, n):
        self._c, self.n = cols, n

    def cols(self):
        return (abi.Col * len(self._c))(*self._c)

    def NumRows(self):
        return self.n


def _mmm(v):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))


def run_collector(ctx, name, cols, types, n, reps, bytes_per_row, depth=5, width=2048):
    ev, wall, last = [], [], None
    for it in range(reps + 1):
        with AnalyzeCollector(ctx, types, 10000, 10000, depth, width, wrap_bytes=True, seed=1) as a:
            ctx.sync()
            t0 = time.perf_counter()
            a.push(Cols(cols, n))
            last = a.finish()
            t1 = time.perf_counter()
            if it:
                ev.append(a.stats()["kernel_ms"])
                wall.append((t1 - t0) * 1e3)
    med = float(np.median(ev))
    line = "collector %-16s events %s ms   push + finish wall %s ms   %3d B/row = %.4f of 8 TB/s   %.1f Mrows/s   NDV estimate %s" % (
        name, _mmm(ev), _mmm(wall), bytes_per_row, bytes_per_row * n / (med * HBM_BYTES_PER_MS), n / med / 1e3, [c.FMSketch.NDV() for c in last])
    return line, {"case": name, "event_ms": ev, "wall_ms": wall, "bytes_per_row": bytes_per_row}


def np_rotl(x, r):
    return (x << U(r)) | (x >> U(64 - r))


def np_fmix(k):
    k = k ^ (k >> U(33))
    k = k * U(0xff51afd7ed558ccd)
    k = k ^ (k >> U(33))
    k = k * U(0xc4ceb9fe1a85ec53)
    return k ^ (k >> U(33))


def host_collect(v, depth, width, max_fm):
    """numpy: varint datum of every int64, murmur3 x64_128 (tail path), CM counters, the canonical FM set"""
    with np.errstate(over="ignore"):
        x = ((v << np.int64(1)) ^ (v >> np.int64(63))).view(U)
        nb = np.ones(len(v), np.int64)  # bytes of the varint: one per started 7-bit group
        for k in range(1, 10):
            nb += (x >> U(7 * k)) != 0
        lo = np.full(len(v), 8, U)
        hi = np.zeros(len(v), U)
        for k in range(10):
            byte = ((x >> U(7 * k)) & U(0x7f)) | np.where(k + 1 < nb, U(0x80), U(0))
            byte = np.where(k < nb, byte, U(0))
            if k < 7:
                lo |= byte << U(8 * (k + 1))
            else:
                hi |= byte << U(8 * (k - 7))
        ln = (nb + 1).astype(U)
        k1 = np_rotl(lo * U(0x87c37b91114253d5), 31) * U(0x4cf5ad432745937f)
        k2 = np_rotl(hi * U(0x4cf5ad432745937f), 33) * U(0x87c37b91114253d5)
        h1, h2 = k1 ^ ln, k2 ^ ln
        h1 = h1 + h2
        h2 = h2 + h1
        h1, h2 = np_fmix(h1), np_fmix(h2)
        h1 = h1 + h2
        h2 = h2 + h1
        cm = np.stack([np.bincount(((h1 + h2 * U(i)) % U(width)).astype(np.int64), minlength=width) for i in range(depth)])
        hs, mask = np.unique(h1), U(0)
        while len(hs) > max_fm:
            mask = mask * U(2) + U(1)
            hs = hs[(hs & mask) == 0]
    return cm, int(mask), hs


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1e8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--host-rows", default="1e7")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, hn = int(float(a.rows)), int(float(a.host_rows))
    lines = ["%d device-resident rows; CM 5 x 2048, FM 10000, 10000 samples; median [min .. max] of %d passes after one warm-up" % (n, a.reps)]
    results = []
    with _lib.Context(0) as ctx:
        ptr = [ctx.alloc(n * 8 + 64) for _ in range(4)]
        offs = ctx.alloc((n + 1) * 8 + 64)
        try:
            ctx.gen_column(spec(abi.GEN_SEQ, 0), n, ptr[0])
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 1, 1000), n, ptr[1])
            ctx.gen_column(spec(abi.GEN_RAND_F64, 2), n, ptr[2])
            ctx.gen_column(spec(abi.GEN_RAND_MOD, 3, 1000000), n, ptr[3])
            ctx.h2d(offs, np.arange(n + 1, dtype=np.int64) * 8)
            cols = [dev_col(ptr[0], abi.I64, n), dev_col(ptr[1], abi.I64, n), dev_col(ptr[2], abi.F64, n), dev_col(ptr[3], abi.BYTES, n, offs)]
            types = [abi.I64, abi.I64, abi.F64, abi.BYTES]
            for i, name in enumerate(["uniq", "k1000", "real", "str"]):
                line, r = run_collector(ctx, name, [cols[i]], [types[i]], n, a.reps, 16 if types[i] == abi.BYTES else 8)
                lines.append(line)
                results.append(r)
                print(line, flush=True)
            line, r = run_collector(ctx, "four columns", cols, types, n, a.reps, 40)
            lines.append(line)
            results.append(r)
            print(line, flush=True)
            k3 = ctx.alloc(n * 8 + 64)  # three values: every lane of a wave meets one of three counters per sketch row
            try:
                ctx.gen_column(spec(abi.GEN_RAND_MOD, 4, 3), n, k3)
                for name, d, w in (("k3", 5, 2048), ("k3, no CM", 0, 0)):
                    line, r = run_collector(ctx, name, [dev_col(k3, abi.I64, n)], [abi.I64], n, a.reps, 8, depth=d, width=w)
                    lines.append(line)
                    results.append(r)
                    print(line, flush=True)
            finally:
                ctx.free(k3)
            for name, i in (("k1000, no CM", 1), ("uniq, no CM", 0)):
                line, r = run_collector(ctx, name, [cols[i]], [types[i]], n, a.reps, 8, depth=0, width=0)
                lines.append(line)
                results.append(r)
                print(line, flush=True)
            scan, walk, wall, st = [], [], [], None
            for it in range(a.reps + 1):
                with SortedBuilder(ctx, abi.I64, 256) as b:
                    ctx.sync()
                    t0 = time.perf_counter()
                    _lib.check(ctx.lib.tsq_sorted_hist_push(b.h, C.byref(cols[0]), n), b.h)
                    h = b.Hist()
                    t1 = time.perf_counter()
                    st = b.stats()
                    if it:
                        scan.append(st["scan_ms"])
                        walk.append(st["walk_ms"])
                        wall.append((t1 - t0) * 1e3)
            assert h.TotalRowCount() == n and h.NDV == n
            line = ("sorted histogram uniq, 256 buckets: scan %s ms (8 + 1 + 1 + 1 + 8 B/row = %.4f of 8 TB/s)   walk %s ms, %d searches, %d buckets   push + finish wall %s ms" %
                    (_mmm(scan), 19 * n / (float(np.median(scan)) * HBM_BYTES_PER_MS), _mmm(walk), st["steps"], h.Len(), _mmm(wall)))
            lines.append(line)
            results.append({"case": "sorted_hist", "scan_ms": scan, "walk_ms": walk, "wall_ms": wall, "steps": st["steps"], "buckets": h.Len()})
            print(line, flush=True)
            # the host leg, on the first host-rows rows of the same columns
            hn = min(hn, n)
            for name, i in (("uniq", 0), ("k1000", 1)):
                v = np.zeros(hn, np.int64)
                ctx.d2h(v, ptr[i])
                t0 = time.perf_counter()
                cm, mask, hs = host_collect(v, 5, 2048, 10000)
                t1 = time.perf_counter()
                with AnalyzeCollector(ctx, [abi.I64], 0, 10000, 5, 2048) as c:
                    c.push(Cols([dev_col(ptr[i], abi.I64, hn)], hn))
                    g = c.finish()[0]
                assert (g.CMSketch.table == cm).all() and g.FMSketch.mask == mask and sorted(g.FMSketch.hashset) == hs.tolist(), "host and GPU sketches differ"
                line = "host numpy %-6s %d rows: %.1f ms = %.2f Mrows/s, one process (sketches equal the GPU's on these rows)" % (name, hn, (t1 - t0) * 1e3, hn / (t1 - t0) / 1e6)
                lines.append(line)
                results.append({"case": "host_" + name, "rows": hn, "ms": (t1 - t0) * 1e3})
                print(line, flush=True)
        finally:
            for p in ptr + [offs]:
                ctx.free(p)
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")
            f.write(json.dumps(results) + "\n")
    print(json.dumps({"bench": "analyze", "cases": len(results)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
