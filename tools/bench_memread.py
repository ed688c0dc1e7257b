#!/usr/bin/env python3
"""Read your own writes on a device-resident transaction buffer: tsq_membuf_scan / scan_points + tsq_membuf_fetch, tsq_membuf_dirty +
dirty_fetch, tsq_unionscan_create_dev and the whole gpu_pipeline.memTableReader (csrc/tsq_memread.hip), whole calls, beside
yardsticks from the same run:
  (a) tsq_copy_d2d of the fetched bytes (keys, values, two offset arrays): the floor;
  (b) tsq_mvcc_scan + tsq_mvcc_fetch over a store that holds the same keys with one version each (the buffer's own finished arrays
      handed to tsq_mvcc_create): the same search and copy, plus version resolution;
  (c) tsq_unionscan_create (the host-built set) on the same handles as tsq_unionscan_create_dev;
  (d) the host path — MemBuffer.entries() + a Python loop over the ranges — on --host-keys keys, one core.
The buffer: --keys record keys (19 bytes) of ascending handles with 38-byte rowcodec rows (two 8-byte integers and a 7-byte string), a
tenth of them deleted afterwards.  Reads: one full range ascending and descending; 2^10 ranges; 2^20 point reads, half of them misses.
Each figure is the median [min .. max] of --reps whole calls after a warm-up (host clock around calls that end in a device
synchronise).  After every timed call the pair count and 4096 sampled pairs (64 runs of 64: key bytes, value bytes, both offsets) are
compared with a numpy restatement; the tool exits non-zero on a mismatch.  No time is a pass/fail gate.
   python tools/bench_memread.py [--keys 1e7] [--host-keys 1e6] [--handles 1e6] [--reps 5] [--out profiles/memread_ab.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mvcc_scan import HBM_BYTES_PER_MS, SIGN, TID, VLEN, mmm  # noqa: E402
from bench_mvcc_scan import record_keys as _record_keys  # noqa: E402
from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import expression as E  # noqa: E402
from tinysql_amd import gpu_pipeline as P  # noqa: E402
from tinysql_amd import kv  # noqa: E402
from tinysql_amd import mvcc as M  # noqa: E402
from tinysql_amd import rowcodec as RC  # noqa: E402
from tinysql_amd import tablecodec as TC  # noqa: E402
from tinysql_amd.chunk import Chunk, Column, StrColumn  # noqa: E402
from tinysql_amd.dupcheck import DevArray  # noqa: E402
from tinysql_amd.executor import unionscan_cfg  # noqa: E402

LINES, FAILED = [], []
A_BASE = 1 << 40
COLUMNS = [RC.ColInfo(1, RC.TypeLonglong, 0, True), RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(3, RC.TypeLonglong), RC.ColInfo(4, RC.TypeVarchar)]


def record_keys(handles):
    """19-byte record keys of table TID (the table id as EncodeInt writes it: tsq_membuf_dirty looks the table up by it)"""
    out = _record_keys(handles)
    out[:, 1:9] = (np.array([TID], dtype=np.uint64) ^ SIGN).astype(">u8").view(np.uint8)
    return out


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps, after=None):
    """median material of `reps` calls after a warm-up; after(result) runs outside the clock after EVERY call"""
    out = []
    for rep in range(reps + 1):
        t0 = time.perf_counter()
        r = fn()
        ms = (time.perf_counter() - t0) * 1e3
        if rep:
            out.append(ms)
        if after:
            after(r)
    return out


class World:
    """the finished buffer and the numpy restatement of what it holds"""

    def __init__(self, ctx, n):
        self.ctx, self.n = ctx, n
        self.hs = np.arange(n, dtype=np.int64) * 3 - n  # ascending, both signs; h + 1 is never a handle
        self.keys = record_keys(self.hs)
        a, b = A_BASE + (np.arange(n, dtype=np.int64) % 1000), (1 << 41) + np.arange(n, dtype=np.int64)
        base = [b"s%06d" % i for i in range(min(n, 1000000))]
        s = StrColumn((base * (n // len(base) + 1))[:n])
        vals, offs = TC.EncodeRow(ctx, Chunk([Column(abi.I64, a), Column(abi.I64, b), s]), [2, 3, 4])
        assert (np.diff(offs) == VLEN).all(), "the generated rows are not %d bytes each" % VLEN
        self.a, self.vals = a, vals.reshape(n, VLEN)
        self.deleted = np.zeros(n, dtype=bool)
        self.deleted[5::10] = True
        self.put_idx = np.flatnonzero(~self.deleted)
        self.mb = kv.MemBuffer(ctx)
        dk, dv = DevArray(ctx, self.keys.reshape(-1)), DevArray(ctx, vals)
        dvo = DevArray(ctx, np.arange(n + 1, dtype=np.int64) * VLEN)
        dd = DevArray(ctx, np.ascontiguousarray(self.keys[self.deleted]).reshape(-1))
        try:
            self.mb.set_packed(dk.p, None, 19 * n, n, dv.p, dvo.p, VLEN * n, device=True)
            self.mb.delete_packed(dd.p, None, 19 * int(self.deleted.sum()), int(self.deleted.sum()), device=True)
        finally:
            for x in (dk, dv, dvo, dd):
                x.free()
        res = self.mb.finish()
        assert (res["n_entries"], res["dels"]) == (n, int(self.deleted.sum())), res

    def expect_ranges(self, bounds, desc):
        """bounds: (lo, hi) entry ordinals per range -> the entry ordinals of the pairs in result order, the positions, the skipped deletes"""
        segs = [self.put_idx[np.searchsorted(self.put_idx, lo):np.searchsorted(self.put_idx, hi)] for lo, hi in bounds]
        idx = np.concatenate(segs) if segs else np.zeros(0, np.int64)
        positions = int(sum(max(hi - lo, 0) for lo, hi in bounds))
        return (idx[::-1] if desc else idx), positions, positions - idx.size

    def check(self, label, pairs, idx, positions, dels, rng):
        """the counts, and 64 runs of 64 pairs read back: key bytes, value bytes and both offset arrays"""
        ok = (pairs.n, pairs.key_bytes, pairs.value_bytes) == (idx.size, 19 * idx.size, VLEN * idx.size)
        ok = ok and pairs.scan["positions"] == positions and pairs.scan["skipped_dels"] == dels
        for _ in range(64 if ok and idx.size else 0):
            o = int(rng.integers(0, max(idx.size - 64, 1)))
            m = min(64, idx.size - o)
            k, v = np.zeros(19 * m, np.uint8), np.zeros(VLEN * m, np.uint8)
            ko, vo = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
            self.ctx.d2h(k, pairs.keys.p + 19 * o)
            self.ctx.d2h(v, pairs.values.p + VLEN * o)
            self.ctx.d2h(ko, pairs.key_offsets.p + 8 * o)
            self.ctx.d2h(vo, pairs.value_offsets.p + 8 * o)
            e = idx[o:o + m]
            ok = ok and np.array_equal(k.reshape(m, 19), self.keys[e]) and np.array_equal(v.reshape(m, VLEN), self.vals[e])
            ok = ok and np.array_equal(ko, 19 * np.arange(o, o + m + 1)) and np.array_equal(vo, VLEN * np.arange(o, o + m + 1))
        if not ok:
            FAILED.append(label)
        return ok


def bench_scan(w, label, rb, ro, n_ranges, desc, idx, positions, dels, reps, store):
    """the buffer scan (scan + fetch, whole call) beside (a) the copy floor and (b) the MVCC read of the same ranges"""
    ctx, rng = w.ctx, np.random.default_rng(7)
    checks = []

    def after(p):
        checks.append(w.check(label, p, idx, positions, dels, rng))
        p.free()
    ms = timed(lambda: w.mb.scan_packed(rb, ro, n_ranges, desc), reps, after)
    nbytes = idx.size * (19 + VLEN + 16) + 16
    src, dst = ctx.alloc(nbytes + 64), ctx.alloc(nbytes + 64)

    def copy():
        _lib.check(ctx.lib.tsq_copy_d2d(ctx.h, C.c_void_p(dst), C.c_void_p(src), nbytes), ctx.h)
        ctx.sync()
    floor = timed(copy, reps)
    ctx.free(src)
    ctx.free(dst)
    flags = np.zeros(max(n_ranges, 1), dtype=np.uint32)
    mv_ok = []

    def mv_after(p):
        mv_ok.append(p.n == idx.size)
        p.free()
    # (a descending MVCC read takes the ranges reversed and yields each descending: the same sequence as the buffer's whole reverse)
    mrb, mro = (rb, ro) if not desc else reverse_ranges(rb, ro, n_ranges)
    mv = timed(lambda: store.scan_packed(mrb, mro, flags[:n_ranges], 1 << 40, desc), reps, mv_after)
    if not all(mv_ok):
        FAILED.append(label + " (mvcc count)")
    m, moved = float(np.median(ms)), 2 * nbytes + positions
    say("%-26s | %8d pairs of %9d positions | scan+fetch %s | (a) copy %s | / (a) %6.2f | (b) mvcc %s | / (b) %5.2f | %5.2f %% of 8 TB/s | %s" %
        (label, idx.size, positions, mmm(ms), mmm(floor), m / float(np.median(floor)), mmm(mv), m / float(np.median(mv)), 100 * moved / (m * HBM_BYTES_PER_MS),
         "count and sampled pairs right" if all(checks) else "WRONG"))
    return m


def reverse_ranges(rb, ro, n):
    cells = [rb[ro[2 * r]:ro[2 * r + 2]] for r in range(n)][::-1]
    lens = [(int(ro[2 * r + 1] - ro[2 * r]), int(ro[2 * r + 2] - ro[2 * r + 1])) for r in range(n)][::-1]
    out = np.concatenate(cells) if cells else np.zeros(0, np.uint8)
    return out, np.concatenate([[0], np.cumsum([x for p in lens for x in p])]).astype(np.int64)


def bench_points(w, reps, store):
    ctx, rng = w.ctx, np.random.default_rng(11)
    n = 1 << 20
    pick = rng.integers(0, w.n, n)
    miss = rng.random(n) < 0.5
    keys = record_keys(w.hs[pick] + miss.astype(np.int64))  # h + 1 is never in the buffer
    hit = ~miss & ~w.deleted[pick]
    idx = pick[hit]
    positions, dels = int((~miss).sum()), int((~miss & w.deleted[pick]).sum())
    dk = DevArray(ctx, keys.reshape(-1))
    checks = []

    def after(p):
        checks.append(w.check("points", p, idx, positions, dels, rng))
        p.free()
    try:
        ms = timed(lambda: w.mb.scan_points_packed(dk.p, None, 19 * n, n, device=True), reps, after)
    finally:
        dk.free()
    rb = keys.reshape(-1)
    ro = np.repeat(np.arange(n + 1, dtype=np.int64) * 19, 2)[1:]  # [key, empty end) per point
    flags = np.full(n, abi.MVCC_POINT, dtype=np.uint32)
    mv_ok = []

    def mv_after(p):
        mv_ok.append(p.n == idx.size)
        p.free()
    mv = timed(lambda: store.scan_packed(rb, ro, flags, 1 << 40), reps, mv_after)
    if not all(mv_ok):
        FAILED.append("points (mvcc count)")
    m = float(np.median(ms))
    say("%-26s | %8d pairs of %9d keys (device keys) | scan+fetch %s | (b) mvcc Get, host keys %s | / (b) %5.2f | %s" %
        ("2^20 points, half misses", idx.size, n, mmm(ms), mmm(mv), m / float(np.median(mv)), "count and sampled pairs right" if all(checks) else "WRONG"))


def bench_dirty(w, reps):
    ctx = w.ctx
    want_a, want_d = w.hs[~w.deleted], w.hs[w.deleted]
    oks = []

    def after(r):
        a, na, d, nd = r
        ok = (na, nd) == (want_a.size, want_d.size)
        if ok:
            rng = np.random.default_rng(13)
            for arr, want in ((a, want_a), (d, want_d)):
                m = min(4096, want.size)
                o = int(rng.integers(0, want.size - m + 1))
                got = np.zeros(m, np.int64)
                ctx.d2h(got, arr + 8 * o)
                ok = ok and np.array_equal(got, want[o:o + m])
        oks.append(ok)
        ctx.free(a)
        ctx.free(d)
    ms = timed(lambda: w.mb.dirty_handles(TID), reps, after)
    if not all(oks):
        FAILED.append("dirty")
    m = float(np.median(ms))
    moved = w.n * (19 + 1 + 16) + w.n * 8  # the keys, ops and offsets read once, the handles written once
    say("%-26s | %d added + %d deleted handles | dirty + dirty_fetch %s | %5.2f %% of 8 TB/s | %s" %
        ("dirty handles of the table", want_a.size, want_d.size, mmm(ms), 100 * moved / (m * HBM_BYTES_PER_MS), "counts and sampled handles right" if all(oks) else "WRONG"))


def bench_create(ctx, n, reps):
    rng = np.random.default_rng(17)
    hs = rng.permutation(4 * n)[:n].astype(np.int64) - 2 * n
    added, deleted = hs[: n // 2].copy(), hs[n // 2:].copy()
    cfg = unionscan_cfg([abi.I64, abi.I64], [], 0, False, 1024)
    da, dd = DevArray(ctx, added), DevArray(ctx, deleted)
    lib = ctx.lib

    def dev():
        h = C.c_void_p()
        _lib.check(lib.tsq_unionscan_create_dev(ctx.h, C.byref(cfg), C.c_void_p(da.p), added.size, C.c_void_p(dd.p), deleted.size, C.byref(h)), ctx.h)
        lib.tsq_unionscan_destroy(h)

    def host():
        h = C.c_void_p()
        _lib.check(lib.tsq_unionscan_create(ctx.h, C.byref(cfg), added.ctypes.data_as(C.POINTER(C.c_int64)), added.size, deleted.ctypes.data_as(C.POINTER(C.c_int64)),
                                            deleted.size, C.byref(h)), ctx.h)
        lib.tsq_unionscan_destroy(h)
    try:
        a, b = timed(dev, reps), timed(host, reps)
    finally:
        da.free()
        dd.free()
    say("%-26s | %d handles (create + destroy) | tsq_unionscan_create_dev %s | (c) tsq_unionscan_create %s | host / dev %6.1f" %
        ("union scan handle set", n, mmm(a), mmm(b), float(np.median(b)) / float(np.median(a))))


def bench_reader(w, reps):
    ctx = w.ctx
    p = b"t" + bytes(w.keys[0, 1:9]) + b"_r"
    ranges = [(p, p[:-1] + b"s")]
    cond = [E.ScalarFunction("gt", E.Column(1, abi.I64), E.Constant(A_BASE + 499))]
    keep = ~w.deleted & (w.a > A_BASE + 499)
    want_h = w.hs[keep]
    oks = []

    def after(chk):
        ok = chk.NumRows() == want_h.size
        if ok:
            o, m = want_h.size // 3, min(4096, want_h.size - want_h.size // 3)
            got = np.zeros(m, np.int64)
            ctx.d2h(got, chk.columns[0].data + 8 * o)
            ok = np.array_equal(got, want_h[o:o + m])
        oks.append(ok)
        chk.free()
    ms = timed(lambda: P.memTableReader(ctx, w.mb, COLUMNS, ranges, False, cond), reps, after)
    if not all(oks):
        FAILED.append("memTableReader")
    say("%-26s | %d of %d rows kept (scan, rowkeys + rowcodec decode, a > c filter, compact) | whole call %s | %s" %
        ("memTableReader", want_h.size, w.n, mmm(ms), "row count and sampled handles right" if all(oks) else "WRONG"))


def host_yardstick(ctx, n):
    """(d) what a host has to do today: export the buffer, walk the ranges in Python"""
    w = World(ctx, n)
    try:
        t0 = time.perf_counter()
        ents = w.mb.entries()
        t1 = time.perf_counter()
        lo, hi = bytes(w.keys[0]), bytes(w.keys[-1]) + b"\x00"
        pairs = [(k, v) for op, k, v in ents if lo <= k < hi and op == abi.MVCC_OP_PUT]
        t2 = time.perf_counter()
        assert len(pairs) == w.put_idx.size
        say("(d) the host path on %d keys, one core: MemBuffer.entries() %.1f ms + the Python loop over one full range %.1f ms = %.3g keys/s" %
            (n, (t1 - t0) * 1e3, (t2 - t1) * 1e3, n / (t2 - t0)))
    finally:
        w.mb.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=float, default=1e7)
    ap.add_argument("--host-keys", type=float, default=1e6)
    ap.add_argument("--handles", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    n = int(a.keys)
    say("tools/bench_memread.py --keys %g --host-keys %g --handles %g --reps %d" % (a.keys, a.host_keys, a.handles, a.reps))
    say("ms per whole call, median [min .. max]; the % column: (fetched bytes read + written + one op byte per position) / time, against 8 TB/s")
    say()
    with _lib.Context(0) as ctx:
        w = World(ctx, n)
        req = w.mb.request()
        cts = DevArray(ctx, np.full(n, 5, dtype=np.uint64))
        store = M.MvccStore(ctx, dict(keys=(req.keys, req.key_bytes), key_offsets=(req.key_offsets, n + 1), commit_ts=(cts.p, n), types=(req.ops, n),
                                      values=(req.values, req.value_bytes), value_offsets=(req.value_offsets, n + 1)), device=True)
        cts.free()
        try:
            say("== %d record keys, %d-byte rows, %d of them deleted" % (n, VLEN, int(w.deleted.sum())))
            prefix = b"t" + bytes(w.keys[0, 1:9]) + b"_r"  # the table's record range: ["t{tid}_r", "t{tid}_s")
            rb, ro = np.frombuffer(prefix + prefix[:-1] + b"s", dtype=np.uint8).copy(), np.array([0, 11, 22], dtype=np.int64)
            for desc in (False, True):
                idx, pos, dels = w.expect_ranges([(0, n)], desc)
                bench_scan(w, "one full range, %s" % ("desc" if desc else "asc"), rb, ro, 1, desc, idx, pos, dels, a.reps, store)
            cuts = np.linspace(0, n, (1 << 10) + 1).astype(np.int64)
            bounds = [(int(lo), int(lo + (hi - lo) * 3 // 4)) for lo, hi in zip(cuts[:-1], cuts[1:])]  # 2^10 ranges with gaps between them
            ends = np.stack([w.keys[[b[0] for b in bounds]], w.keys[[b[1] for b in bounds]]], axis=1)
            rb, ro = ends.reshape(-1), np.arange(2 * len(bounds) + 1, dtype=np.int64) * 19
            for desc in (False, True):
                idx, pos, dels = w.expect_ranges(bounds, desc)
                bench_scan(w, "2^10 ranges, %s" % ("desc" if desc else "asc"), rb, ro, len(bounds), desc, idx, pos, dels, a.reps, store)
            bench_points(w, a.reps, store)
            bench_dirty(w, a.reps)
            bench_reader(w, a.reps)
            bench_create(ctx, int(a.handles), a.reps)
        finally:
            store.close()
            w.mb.close()
        say()
        host_yardstick(ctx, int(a.host_keys))
    if FAILED:
        say("FAILED: a wrong count or sampled pair: %s" % ", ".join(sorted(set(FAILED))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(1 if FAILED else 0)


if __name__ == "__main__":
    main()
