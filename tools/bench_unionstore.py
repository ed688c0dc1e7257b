#!/usr/bin/env python3
"""A transaction's merged read on the device: tsq_unionstore_scan / get + tsq_unionstore_fetch (csrc/tsq_unionstore.hip), whole calls,
beside yardsticks from the same run:
  (a) tsq_mvcc_scan + tsq_mvcc_fetch of the same store alone;
  (b) tsq_membuf_scan + tsq_membuf_fetch of the same buffer alone — (a) + (b) is the natural floor of the merged read;
  (c) tsq_copy_d2d of the fetched bytes (keys, values, two offset arrays);
  (d) for DeviceTable.from_union / from_pairs: the existing host constructor on the downloaded pairs.
The store is bench_mvcc_scan.py's "v1": --keys record keys (19 bytes, handles 3 k) with 38-byte values, one version per key.  The
buffers hold 1e3, 1e6 and 1e7 entries spread evenly over the store's key space: half new handles (3 k + 1), 40 % overwrites of stored
handles, 10 % deletes.  Reads: one full range ascending and descending; 2^10 ranges; limit = 1; 2^20 point reads (a third in the
buffer, a third only in the store, a third nowhere); the handle without a buffer (the snapshot route).
Each figure is the median [min .. max] of --reps whole calls after a warm-up (host clock around calls that end in a device
synchronise).  After every timed call the counts, and for the full-range reads 4096 sampled pairs (64 runs of 64: key bytes, value
bytes, both offsets, the from_buffer flags), are compared with a numpy restatement; the tool exits non-zero on a mismatch.  No time is
a pass/fail gate.
   python tools/bench_unionstore.py [--keys 1e8] [--buffers 1e3,1e6,1e7] [--table-keys 1e7] [--reps 5] [--out profiles/unionstore_ab.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mvcc_scan import HBM_BYTES_PER_MS, READ_TS, VLEN, Store, mmm, record_keys  # noqa: E402
from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import coprocessor  # noqa: E402
from tinysql_amd import kv  # noqa: E402
from tinysql_amd.dupcheck import DevArray  # noqa: E402

LINES, FAILED = [], []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def timed(fn, reps, after=None):
    """`reps` calls after a warm-up; after(result) runs outside the clock after EVERY call"""
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


def store_values(k):
    """the 38 bytes the store holds for key ordinals k (bench_mvcc_scan.Store: the entry's index, then a pattern)"""
    v = np.empty((k.size, VLEN), dtype=np.uint8)
    v[:, :8] = k.astype("<u8").view(np.uint8).reshape(-1, 8)
    v[:, 8:] = (np.arange(VLEN - 8, dtype=np.uint8) + 65)[None, :]
    return v


def buffer_values(i):
    v = np.empty((i.size, VLEN), dtype=np.uint8)
    v[:, :8] = (i.astype(np.int64) | (1 << 62)).astype("<u8").view(np.uint8).reshape(-1, 8)
    v[:, 8:] = (np.arange(VLEN - 8, dtype=np.uint8) + 97)[None, :]
    return v


class Buffer:
    """m entries: entry i sits at store ordinal kk[i] = i * (K // m); i % 10 in 0..4: a new handle 3 kk + 1, 5..8: an overwrite of 3 kk,
    9: a delete of 3 kk — and the numpy restatement of the merged table"""

    def __init__(self, ctx, K, m):
        self.ctx, self.K, self.m = ctx, K, m
        i = np.arange(m, dtype=np.int64)
        self.g = K // m
        self.kk = i * self.g
        kind = i % 10
        self.new, self.over, self.dele = kind < 5, (kind >= 5) & (kind < 9), kind == 9
        handles = 3 * self.kk + self.new.astype(np.int64)
        keys = record_keys(handles)
        put = ~self.dele
        self.mb = kv.MemBuffer(ctx)
        dk, dv = DevArray(ctx, np.ascontiguousarray(keys[put]).reshape(-1)), DevArray(ctx, buffer_values(i[put]).reshape(-1))
        dvo = DevArray(ctx, np.arange(int(put.sum()) + 1, dtype=np.int64) * VLEN)
        dd = DevArray(ctx, np.ascontiguousarray(keys[self.dele]).reshape(-1))
        try:
            self.mb.set_packed(dk.p, None, 19 * int(put.sum()), int(put.sum()), dv.p, dvo.p, VLEN * int(put.sum()), device=True)
            self.mb.delete_packed(dd.p, None, 19 * int(self.dele.sum()), int(self.dele.sum()), device=True)
        finally:
            for x in (dk, dv, dvo, dd):
                x.free()
        res = self.mb.finish()
        assert (res["n_entries"], res["dels"]) == (m, int(self.dele.sum())), res
        self.n_new, self.n_over, self.n_del = int(self.new.sum()), int(self.over.sum()), int(self.dele.sum())
        self.total = K - self.n_del + self.n_new
        # per entry: the merged pairs before store ordinal kk[i] (exclusive prefix of +1 per new, -1 per delete)
        delta = self.new.astype(np.int64) - self.dele.astype(np.int64)
        self.before = np.concatenate([[0], np.cumsum(delta)])

    def pos(self, k):
        """the merged pairs before store ordinal k (k in [0, K])"""
        e = np.minimum((np.asarray(k, dtype=np.int64) + self.g - 1) // self.g, self.m)  # entries with kk < k
        return np.asarray(k, dtype=np.int64) + self.before[e]

    def expect(self, k0, k1):
        """the merged pairs of store ordinals [k0, k1): (keys [n, 19], values [n, 38], from_buffer [n])"""
        ks, vs, fb = [], [], []
        k = np.arange(k0, k1, dtype=np.int64)
        e = k // self.g
        at = (k % self.g == 0) & (e < self.m)
        ee = np.where(at, e, 0)
        is_new, is_over, is_del = at & self.new[ee], at & self.over[ee], at & self.dele[ee]
        n = k.size
        # two slots per ordinal: the stored (or overwritten) handle, then the new one
        keep = np.stack([~is_del, is_new], axis=1).reshape(-1)
        handles = np.stack([3 * k, 3 * k + 1], axis=1).reshape(-1)[keep]
        vals = np.stack([np.where(is_over[:, None], buffer_values(ee), store_values(k)), buffer_values(ee)], axis=1).reshape(2 * n, VLEN)[keep]
        fbuf = np.stack([is_over, is_new], axis=1).reshape(-1)[keep]
        return record_keys(handles), vals, fbuf.astype(np.uint8)

    def close(self):
        self.mb.close()


def check_samples(ctx, b, p, desc, rng, label):
    ok = (p.n, p.key_bytes, p.value_bytes) == (b.total, 19 * b.total, VLEN * b.total)
    for _ in range(64 if ok else 0):
        k0 = int(rng.integers(0, max(b.K - 64, 1)))
        keys, vals, fb = b.expect(k0, min(k0 + 64, b.K))
        m, o = keys.shape[0], int(b.pos(k0))
        if m == 0:
            continue
        if desc:
            keys, vals, fb, o = keys[::-1], vals[::-1], fb[::-1], b.total - o - m
        k, v, f = np.zeros(19 * m, np.uint8), np.zeros(VLEN * m, np.uint8), np.zeros(m, np.uint8)
        ko, vo = np.zeros(m + 1, np.int64), np.zeros(m + 1, np.int64)
        ctx.d2h(k, p.keys.p + 19 * o)
        ctx.d2h(v, p.values.p + VLEN * o)
        ctx.d2h(ko, p.key_offsets.p + 8 * o)
        ctx.d2h(vo, p.value_offsets.p + 8 * o)
        ctx.d2h(f, p.from_buffer.p + o)
        ok = ok and np.array_equal(k.reshape(m, 19), keys) and np.array_equal(v.reshape(m, VLEN), vals) and np.array_equal(f, fb)
        ok = ok and np.array_equal(ko, 19 * np.arange(o, o + m + 1)) and np.array_equal(vo, VLEN * np.arange(o, o + m + 1))
    if not ok:
        FAILED.append(label)
    return ok


def pack(cells):
    offs = np.zeros(len(cells) + 1, dtype=np.int64)
    offs[1:] = np.cumsum([len(c) for c in cells])
    return np.frombuffer(b"".join(cells), dtype=np.uint8).copy(), offs


def copy_floor(ctx, nbytes, reps):
    src, dst = ctx.alloc(nbytes + 64), ctx.alloc(nbytes + 64)

    def copy():
        _lib.check(ctx.lib.tsq_copy_d2d(ctx.h, C.c_void_p(dst), C.c_void_p(src), nbytes), ctx.h)
        ctx.sync()
    try:
        return timed(copy, reps)
    finally:
        ctx.free(src)
        ctx.free(dst)


def free_after(p):
    p.free()


def run_buffer(ctx, st, m, reps, mv_full):
    K = st.K
    b = Buffer(ctx, K, m)
    us = kv.UnionStore(ctx, st.ms, b.mb, READ_TS)
    rng = np.random.default_rng(5)
    say("== buffer of %d entries (%d new, %d overwrites, %d deletes) over %d store keys: %d merged pairs" % (m, b.n_new, b.n_over, b.n_del, K, b.total))
    try:
        full_rb, full_ro = pack([b"", b""])
        mem = timed(lambda: b.mb.scan_packed(full_rb, full_ro, 1, False), reps, free_after)
        nbytes = b.total * (19 + VLEN + 16) + 16
        floor = copy_floor(ctx, nbytes, reps)
        say("   yardsticks: (a) tsq_mvcc_scan + fetch %s | (b) tsq_membuf_scan + fetch %s | (c) copy of %.2f GB %s" % (mmm(mv_full), mmm(mem), nbytes / 1e9, mmm(floor)))
        ab = float(np.median(mv_full)) + float(np.median(mem))
        for desc in (False, True):
            checks = []

            def after(p):
                checks.append(check_samples(ctx, b, p, desc, rng, "full %d desc=%d" % (m, desc)))
                p.free()
            ms = timed(lambda: us.scan_packed(full_rb, full_ro, 1, desc), reps, after)
            med = float(np.median(ms))
            say("   one full range, %-10s | scan+fetch %s | / (a)+(b) %6.2f | / (a) %6.2f | / (c) %6.2f | %5.2f %% of 8 TB/s | %s" %
                ("descending" if desc else "ascending", mmm(ms), med / ab, med / float(np.median(mv_full)), med / float(np.median(floor)),
                 100 * 2 * nbytes / (med * HBM_BYTES_PER_MS), "count and sampled pairs right" if all(checks) else "WRONG"))
        # 2^10 ranges: every second 1/2048th of the key space
        R = 1 << 10
        w = K // (2 * R)
        los = np.arange(R, dtype=np.int64) * 2 * w
        bk = record_keys(3 * np.stack([los, los + w], axis=1).reshape(-1))
        rb, ro = bk.reshape(-1).copy(), np.arange(2 * R + 1, dtype=np.int64) * 19
        want = (b.pos(los + w) - b.pos(los)).tolist()
        for desc in (False, True):
            ok = []

            def after_r(p):
                ok.append(p.counts == want and p.n == sum(want))
                p.free()
            ms = timed(lambda: us.scan_packed(rb, ro, R, desc, want_counts=True), reps, after_r)
            flags = np.zeros(R, dtype=np.uint32)
            mv = timed(lambda: st.ms.scan_packed(rb, ro, flags, READ_TS, desc), reps, free_after)
            if not all(ok):
                FAILED.append("ranges %d desc=%d" % (m, desc))
            say("   2^10 ranges, %-13s | %9d pairs | scan+fetch %s | (a) mvcc, same ranges %s | / (a) %6.2f | %s" %
                ("descending" if desc else "ascending", sum(want), mmm(ms), mmm(mv), float(np.median(ms)) / float(np.median(mv)), "counts right" if all(ok) else "WRONG"))
        # limit = 1
        ok = []

        def after_l(p):
            first = b.expect(0, 1)[0]
            k = np.zeros(19, np.uint8)
            if p.n == 1:
                ctx.d2h(k, p.keys.p)
            ok.append(p.n == 1 and np.array_equal(k, first[0]))
            p.free()
        ms = timed(lambda: us.scan_packed(full_rb, full_ro, 1, False, 1), reps, after_l)
        if not all(ok):
            FAILED.append("limit %d" % m)
        say("   one full range, limit = 1   | scan+fetch %s | %s   (every position is still resolved and placed: the limit cuts the output only)" %
            (mmm(ms), "the first pair" if all(ok) else "WRONG"))
        # 2^20 point reads
        n = 1 << 20
        i = rng.integers(0, m, n)
        k = rng.integers(0, K, n)
        which = np.arange(n) % 3
        in_buf = 3 * b.kk[i] + b.new[i].astype(np.int64)  # a buffer key (a delete among them: not found)
        store_only = 3 * np.where(k % b.g == 0, np.where(k == 0, 1, k - 1), k)  # (a store ordinal the buffer does not touch)
        if b.g == 1:
            store_only = in_buf
        handles = np.where(which == 0, in_buf, np.where(which == 1, store_only, 3 * k + 2))
        found = np.where(which == 0, ~b.dele[i], which == 1) if b.g > 1 else np.where(which == 2, False, ~b.dele[i])
        dk = DevArray(ctx, record_keys(handles).reshape(-1))
        ok = []

        def after_p(r):
            f, p = r
            ok.append(np.array_equal(f.astype(bool), found) and p.n == int(found.sum()))
            p.free()
        try:
            ms = timed(lambda: us.get_packed(dk.p, None, 19 * n, n, device=True), reps, after_p)
        finally:
            dk.free()
        if not all(ok):
            FAILED.append("points %d" % m)
        say("   2^20 point reads (device keys) | %8d found | get+fetch %s | %s" % (int(found.sum()), mmm(ms), "every verdict right" if all(ok) else "WRONG"))
        say()
    finally:
        us.close()
        b.close()


def run_table(ctx, st, n_keys, reps):
    """DeviceTable over the first n_keys store keys through a buffer of n_keys / 100 entries: from_pairs on the device-resident pairs of
    the union read against (d) the host constructor on the downloaded pairs"""
    b = Buffer(ctx, n_keys, max(n_keys // 100, 10))
    us = kv.UnionStore(ctx, st.ms, b.mb, READ_TS)
    rng_keys = [bytes(record_keys(np.array([0], dtype=np.int64))[0]), bytes(record_keys(np.array([3 * n_keys], dtype=np.int64))[0])]
    try:
        def on_device():
            t = coprocessor.DeviceTable.from_pairs(ctx, us.scan([tuple(rng_keys)]))
            ctx.sync()
            return t

        def on_host():
            p = us.scan([tuple(rng_keys)])
            try:
                keys, vals, offs = p.keys.read(np.uint8, p.key_bytes), p.values.read(np.uint8, p.value_bytes), p.value_offsets.read(np.int64, p.n + 1)
            finally:
                p.free()
            t = coprocessor.DeviceTable(ctx, keys, vals, offs)
            ctx.sync()
            return t
        ok = []

        def after(t):
            ok.append(t.n == b.total)
            t.close()
        dev = timed(on_device, reps, after)
        host = timed(on_host, reps, after)
        if not all(ok):
            FAILED.append("table")
        say("== DeviceTable of %d rows from the union read: scan + from_pairs %s | (d) scan + download + host constructor %s | (d) / device %6.1f | %s" %
            (b.total, mmm(dev), mmm(host), float(np.median(host)) / float(np.median(dev)), "row counts right" if all(ok) else "WRONG"))
        say()
    finally:
        us.close()
        b.close()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=float, default=1e8)
    ap.add_argument("--buffers", default="1e3,1e6,1e7")
    ap.add_argument("--table-keys", type=float, default=1e7)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    a = ap.parse_args()
    K = int(a.keys)
    say("tools/bench_unionstore.py --keys %g --buffers %s --table-keys %g --reps %d" % (a.keys, a.buffers, a.table_keys, a.reps))
    say("ms per whole call, median [min .. max]; the %% column: 2 x the fetched bytes (read once, written once) against 8 TB/s")
    say()
    with _lib.Context(0) as ctx:
        st = Store(ctx, "v1", K, 0)
        try:
            full_rb, full_ro = pack([b"", b""])
            flags = np.zeros(1, dtype=np.uint32)
            mv_ok = []

            def mv_after(p):
                mv_ok.append(p.n == K)
                p.free()
            mv_full = timed(lambda: st.ms.scan_packed(full_rb, full_ro, flags, READ_TS), a.reps, mv_after)
            # the handle without a buffer: the snapshot route
            us = kv.UnionStore(ctx, st.ms, None, READ_TS)
            try:
                fast = timed(lambda: us.scan_packed(full_rb, full_ro, 1), a.reps, mv_after)
                route = us.stats()["last_route"]
            finally:
                us.close()
            if not all(mv_ok) or route != abi.UNION_ROUTE_SNAPSHOT:
                FAILED.append("snapshot route")
            say("== %d store keys, no buffer (mb == NULL, the snapshot route): union scan+fetch %s | (a) tsq_mvcc_scan + fetch %s | / (a) %5.2f | %s" %
                (K, mmm(fast), mmm(mv_full), float(np.median(fast)) / float(np.median(mv_full)), "counts right" if all(mv_ok) else "WRONG"))
            say()
            for m in [int(float(x)) for x in a.buffers.split(",") if x]:
                if m <= K:
                    run_buffer(ctx, st, m, a.reps, mv_full)
            run_table(ctx, st, min(int(a.table_keys), K), a.reps)
        finally:
            st.free()
    if FAILED:
        say("FAILED: " + ", ".join(FAILED))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(1 if FAILED else 0)


if __name__ == "__main__":
    main()
