#!/usr/bin/env python3
"""UnionScan on device columns: tsq_unionscan_* (csrc/tsq_unionscan.hip) over a device-resident snapshot, beside what a caller could do
before with the same rows — tsq_chunk_compact of the kept rows, then tsq_sort_* over the concatenation with the added rows — timed
alternately in the same process on the same inputs, results compared.

Workload: --rows snapshot rows (default 1e8) of (BIGINT handle, BIGINT, DOUBLE) in HBM, pushed as chunks of --chunk rows (2^22) and pulled
after every push; a dirty table of D handles (half deleted snapshot handles, half added handles that fall between snapshot handles, each
with an added row), D from --dirty (0, 1e3, 1e6, 1e7).
  table   handle order (no index columns)
  index   one BIGINT index column (non-decreasing, four rows per value), then the handle
  string  table order with an 8-byte string payload column (one dirty size: --string-dirty)
ms = device events around the whole push / pull loop (the host's waits between the launches included: what the caller sees), median
[min .. max] of --reps passes after one warm-up pass per shape; kernel ms = tsq_unionscan_stats.  Algorithmic bytes, computed here: every
input column read once + every output column written once + 8 B per snapshot row for the handle probe; the share is of 8 TB/s.
Yardstick (a): the keep flags are given to it for free (the library has no set probe outside this operator); its time is compact + sort
push + finish + pull.  Yardstick (b): numpy on one host core at --host-rows rows (isin, concatenate, stable argsort, take).
   python tools/bench_union_scan.py [--rows 1e8] [--reps 2] [--dirty 0,1e3,1e6,1e7] [--out profiles/union_scan_ab.txt]"""
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
from tinysql_amd import executor as X  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3


def _mmm(v):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))


def dev_col(data, tp, n, offsets=None):
    c = abi.Col()
    c.data, c.length, c.elem_size, c.type, c.flags, c.offsets = data, n, (-1 if tp == abi.BYTES else 8), tp, abi.COL_DEVICE, offsets
    return c


class Table:
    """n rows in HBM: handle = 2 i, key = i // 4, b = 7 i mod 1000003, c = i / 2, s = the 8 bytes of i (a var-len column)"""

    def __init__(self, ctx, n, with_string):
        self.ctx, self.n = ctx, n
        self.types = [abi.I64, abi.I64, abi.I64, abi.F64] + ([abi.BYTES] if with_string else [])
        self.ptr = [ctx.alloc(n * 8 + 64) for _ in range(5 if with_string else 4)]
        self.offs = ctx.alloc((n + 1) * 8 + 64) if with_string else None
        step = 1 << 24
        for lo in range(0, n, step):
            i = np.arange(lo, min(n, lo + step), dtype=np.int64)
            for k, arr in enumerate(self.cols_of(i * 2, with_string)):
                ctx.h2d(self.ptr[k] + lo * 8, arr)
        if with_string:
            ctx.h2d(self.offs, np.arange(n + 1, dtype=np.int64) * 8)

    @staticmethod
    def cols_of(h, with_string):
        i = h >> 1
        out = [h, i >> 2, (i * 7) % 1000003, i * 0.5]
        return out + [i.copy()] if with_string else out

    def view(self, cols, lo, cnt):
        """tsq_col array of rows [lo, lo + cnt) of the chosen columns"""
        out = []
        for k in cols:
            if self.types[k] == abi.BYTES:
                out.append(dev_col(self.ptr[k], abi.BYTES, cnt, self.offs + 8 * lo))
            else:
                out.append(dev_col(self.ptr[k] + 8 * lo, self.types[k], cnt))
        return (abi.Col * len(out))(*out)

    def free(self):
        for p in self.ptr + ([self.offs] if self.offs else []):
            self.ctx.free(p)


class OutBuf:
    def __init__(self, ctx, types, cap):
        self.ctx, self.types, self.cap = ctx, types, cap
        self.data = [ctx.alloc(cap * 8 + 64) for _ in types]
        self.bm = [ctx.alloc(cap // 8 + 64) for _ in types]
        self.offs = [ctx.alloc((cap + 1) * 8 + 64) if t == abi.BYTES else None for t in types]

    def cols(self):
        out = []
        for k, t in enumerate(self.types):
            c = dev_col(self.data[k], t, self.cap, self.offs[k])
            c.null_bitmap = self.bm[k]
            out.append(c)
        return (abi.Col * len(out))(*out)

    def free(self):
        for p in self.data + self.bm + [o for o in self.offs if o]:
            self.ctx.free(p)


def dirty_of(n, d, seed):
    """d dirty handles: d // 2 deleted snapshot handles and d - d // 2 added handles (odd: between two snapshot handles)"""
    rng = np.random.default_rng(seed)

    def pick(k):  # k distinct row numbers, sorted (without permuting all n of them)
        if k == 0:
            return np.zeros(0, np.int64)
        if 2 * k >= n:
            return np.sort(rng.choice(n, k, replace=False)).astype(np.int64)
        idx = np.unique(rng.integers(0, n, int(k * 1.3) + 64))
        while len(idx) < k:
            idx = np.unique(np.concatenate([idx, rng.integers(0, n, k)]))
        return np.sort(rng.choice(idx, k, replace=False)).astype(np.int64)
    deleted, added = pick(d // 2) * 2, pick(d - d // 2) * 2 + 1
    return deleted, added


class Bench:
    def __init__(self, ctx, n, chunk, reps):
        self.ctx, self.lib, self.n, self.chunk, self.reps = ctx, ctx.lib, n, chunk, reps
        self.lines, self.results = [], []

    def say(self, line, rec=None):
        self.lines.append(line)
        if rec:
            self.results.append(rec)
        print(line, flush=True)

    def union_scan(self, tab, cols, used_index, deleted, added, added_cols, out, keep_handles):
        """one pass: create, set_added, push + pull per chunk, finish, pull; returns (ms, kernel ms, rows out, handles out or None)"""
        ctx, lib = self.ctx, self.lib
        types = [tab.types[k] for k in cols]
        cfg = X.unionscan_cfg(types, used_index, 0, False, 1024)
        d = X.DirtyTable()
        d.addedRows, d.deletedRows = added, deleted  # (anything iterable: unionscan_create sorts them into arrays)
        h = X.unionscan_create(ctx, cfg, d)
        got, rows_out = [], 0
        try:
            keep = []
            from tinysql_amd.chunk import make_cols
            _lib.check(lib.tsq_unionscan_set_added(h, make_cols(added_cols, keep), len(added_cols), len(added)), h)
            oc, n_out, eos = out.cols(), C.c_int64(0), C.c_int32(0)

            def pull_all():
                nonlocal rows_out
                while True:
                    if abi.BYTES in types:  # (the peek sizes nothing here: the buffers hold 8 B per row, what the cells have)
                        vb, pn = (C.c_int64 * len(types))(), C.c_int64(0)
                        _lib.check(lib.tsq_unionscan_peek(h, out.cap, C.byref(pn), vb, len(types)), h)
                    _lib.check(lib.tsq_unionscan_pull(h, oc, len(types), out.cap, C.byref(n_out), C.byref(eos)), h)
                    if n_out.value == 0:
                        return
                    if keep_handles:
                        a = np.zeros(n_out.value, np.int64)
                        ctx.d2h(a, out.data[0])
                        got.append(a)
                    rows_out += n_out.value
            ctx.sync()
            ctx.timer_start()
            for lo in range(0, self.n, self.chunk):
                cnt = min(self.chunk, self.n - lo)
                _lib.check(lib.tsq_unionscan_push(h, tab.view(cols, lo, cnt), len(cols), cnt), h)
                pull_all()
            _lib.check(lib.tsq_unionscan_finish(h), h)
            pull_all()
            ms = ctx.timer_stop_ms()
            kms = C.c_double(0)
            lib.tsq_unionscan_stats(h, None, None, None, C.byref(kms))
        finally:
            lib.tsq_unionscan_destroy(h)
        return ms, kms.value, rows_out, (np.concatenate(got) if got else np.zeros(0, np.int64)) if keep_handles else None

    def compact_sort(self, tab, cols, used_index, flags, added_cols, n_added, out, keep_handles):
        """yardstick (a): tsq_chunk_compact per chunk with the given keep flags (device), the kept rows and the added rows into tsq_sort_*"""
        ctx, lib = self.ctx, self.lib
        types = [tab.types[k] for k in cols]
        cfg = abi.SortCfg()
        cfg.n_cols = len(types)
        for i, t in enumerate(types):
            cfg.col_types[i] = t
        by = list(used_index) + [0]
        cfg.n_keys = len(by)
        for i, c in enumerate(by):
            cfg.key_col[i], cfg.key_desc[i] = c, 0
        cfg.limit_offset, cfg.limit_count, cfg.max_chunk_size = 0, -1, 1024
        h = C.c_void_p()
        _lib.check(lib.tsq_sort_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
        got, rows_out = [], 0
        try:
            from tinysql_amd.chunk import make_cols
            keep = []
            oc, m, n_out, eos = out.cols(), C.c_int64(0), C.c_int64(0), C.c_int32(0)
            ctx.sync()
            ctx.timer_start()
            for lo in range(0, self.n, self.chunk):
                cnt = min(self.chunk, self.n - lo)
                if flags:
                    _lib.check(lib.tsq_chunk_compact(ctx.h, tab.view(cols, lo, cnt), len(cols), cnt, C.c_void_p(flags + lo), oc, C.byref(m)), ctx.h)
                    if m.value:
                        _lib.check(lib.tsq_sort_push(h, oc, len(cols), m.value), h)
                else:
                    _lib.check(lib.tsq_sort_push(h, tab.view(cols, lo, cnt), len(cols), cnt), h)
            if n_added:
                _lib.check(lib.tsq_sort_push(h, make_cols(added_cols, keep), len(added_cols), n_added), h)
            _lib.check(lib.tsq_sort_finish(h), h)
            while True:
                if abi.BYTES in types:
                    vb, pn = (C.c_int64 * len(types))(), C.c_int64(0)
                    _lib.check(lib.tsq_sort_peek(h, out.cap, C.byref(pn), vb, len(types)), h)
                _lib.check(lib.tsq_sort_pull(h, oc, len(types), out.cap, C.byref(n_out), C.byref(eos)), h)
                if n_out.value == 0:
                    break
                if keep_handles:
                    a = np.zeros(n_out.value, np.int64)
                    ctx.d2h(a, out.data[0])
                    got.append(a)
                rows_out += n_out.value
            ms = ctx.timer_stop_ms()
        finally:
            lib.tsq_sort_destroy(h)
        return ms, rows_out, (np.concatenate(got) if got else np.zeros(0, np.int64)) if keep_handles else None

    def case(self, name, tab, cols, used_index, d):
        from tinysql_amd.chunk import Column, StrColumn
        ctx, n = self.ctx, self.n
        types = [tab.types[k] for k in cols]
        deleted, added = dirty_of(n, d, d + len(cols))
        acols_np = Table.cols_of(added, abi.BYTES in tab.types)
        added_cols = [StrColumn([x.tobytes() for x in acols_np[k]]) if tab.types[k] == abi.BYTES else Column(tab.types[k], acols_np[k]) for k in cols]
        flags = None
        if d:
            f = np.ones(n, np.uint8)
            f[deleted >> 1] = 0
            flags = ctx.alloc(n + 64)
            ctx.h2d(flags, f)
        out = OutBuf(ctx, types, self.chunk + len(added) + 64)
        n_var = sum(1 for t in types if t == abi.BYTES)
        row_b = 8 * len(types) + 8 * n_var  # a var-len cell here: 8 B of offset + its 8 bytes
        kept = n - len(deleted)
        alg = n * row_b + len(added) * row_b + (kept + len(added)) * row_b + (8 * n if d else 0)
        try:
            us_ms, us_k, ab_ms, same = [], [], [], None
            for it in range(self.reps + 1):  # pass 0 warms both up and compares the results; the two variants alternate
                first = it == 0
                ms, kms, rows, hs = self.union_scan(tab, cols, used_index, set(deleted.tolist()), set(added.tolist()), added_cols, out, first)
                ms2, rows2, hs2 = self.compact_sort(tab, cols, used_index, flags, added_cols, len(added), out, first)
                assert rows == rows2 == kept + len(added), (rows, rows2, kept + len(added))
                if first:
                    same = bool(np.array_equal(hs, hs2))
                else:
                    us_ms.append(ms)
                    us_k.append(kms)
                    ab_ms.append(ms2)
            med, med2 = float(np.median(us_ms)), float(np.median(ab_ms))
            self.say("%-7s dirty %-8d union scan %s ms (kernels %8.3f)  %6.1f B/row = %.4f of 8 TB/s  %7.1f Mrows/s | compact + sort %s ms  = %.2f x  | same rows: %s" % (
                name, d, _mmm(us_ms), float(np.median(us_k)), alg / n, alg / (med * HBM_BYTES_PER_MS), n / med / 1e3, _mmm(ab_ms), med2 / med, same),
                {"case": name, "dirty": d, "union_scan_ms": us_ms, "kernel_ms": us_k, "compact_sort_ms": ab_ms, "alg_bytes": alg, "same": same})
        finally:
            out.free()
            if flags:
                ctx.free(flags)


def host_leg(b, hn, d):
    deleted, added = dirty_of(hn, d, 3)
    h = np.arange(hn, dtype=np.int64) * 2
    cols = Table.cols_of(h, False)
    acols = Table.cols_of(added, False)
    t0 = time.perf_counter()
    keep = ~np.isin(h, np.concatenate([deleted, added]))
    merged = [np.concatenate([c[keep], a]) for c, a in zip(cols, acols)]
    order = np.argsort(merged[0], kind="stable")
    outc = [c[order] for c in merged]
    t1 = time.perf_counter()
    b.say("host numpy, table order, %d rows, dirty %d: %.1f ms = %.2f Mrows/s, one core (isin, concatenate, stable argsort, take); %d rows out" % (
        hn, d, (t1 - t0) * 1e3, hn / (t1 - t0) / 1e6, len(outc[0])), {"case": "host_numpy", "rows": hn, "dirty": d, "ms": (t1 - t0) * 1e3})


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1e8")
    ap.add_argument("--chunk", type=int, default=1 << 22)
    ap.add_argument("--reps", type=int, default=2)
    ap.add_argument("--dirty", default="0,1e3,1e6,1e7")
    ap.add_argument("--string-dirty", default="1e6")
    ap.add_argument("--host-rows", default="1e7")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n, hn = int(float(a.rows)), int(float(a.host_rows))
    dirty = [int(float(x)) for x in a.dirty.split(",") if x != ""]
    with _lib.Context(0) as ctx:
        b = Bench(ctx, n, a.chunk, a.reps)
        b.say("%d device-resident snapshot rows, %d rows per push, everything pulled after every push; ms = device events around the whole loop, "
              "median [min .. max] of %d passes after a warm-up pass; one merge route (the general one): nothing to A/B between routes" % (n, a.chunk, a.reps))
        tab = Table(ctx, n, True)
        try:
            for d in dirty:
                if d <= n:
                    b.case("table", tab, [0, 2, 3], [], d)
            for d in dirty:
                if d <= n:
                    b.case("index", tab, [0, 1, 3], [1], d)
            sd = int(float(a.string_dirty))
            b.case("string", tab, [0, 2, 3, 4], [], min(sd, n))
        finally:
            tab.free()
        host_leg(b, min(hn, n), min(1000000, hn))
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(b.lines) + "\n")
            f.write(json.dumps(b.results) + "\n")
    print(json.dumps({"bench": "union_scan", "cases": len(b.results)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
