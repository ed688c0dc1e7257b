#!/usr/bin/env python3
"""MVCC range calls on a device-resident store: tsq_mvcc_gc, tsq_mvcc_resolve_lock, tsq_mvcc_scan_lock and tsq_mvcc_delete_range
(csrc/tsq_mvcc_maint.hip) as whole calls, each beside two yardsticks from the same run:
  (a) tsq_copy_d2d of the SURVIVING version arrays (keys, offsets, commitTS, startTS, types, values of the next store): what a rewrite
      must move at least;
  (b) tsq_mvcc_create over the next store's exported device arrays: the rebuild (head flags, ordinals, universe) every apply contains.
The store: the v3 store of tools/bench_mvcc_scan.py, writable — --keys record keys with 1..5 versions each (mean 3), 5 % deletes, 1 %
rollbacks, commitTS 16 .. 87, startTS = commitTS - 1.
  gc            at a safe point above every version, and at the median commitTS
  resolve_lock  of 2^10, 2^16 and 2^22 locks of ONE transaction (Puts, prewritten on keys spread over the store, committed by the
                resolve); the prewrite that makes them is timed too: the write path's apply on the same store
  scan_lock     over the 2^22 locks, the output device resident
  delete_range  of a tenth of the keys, in the middle of the store
Host clock around calls that end in a device synchronise, median [min .. max] of --reps after a warm-up; kernel_ms and mark_ms (the
bound and marking passes in front of the apply) from the call's result.  After every timed call the next store's entry count is held
to the numpy restatement of the call over the whole store, and a sample of keys is read back against the restatement of getValue;
the tool exits non-zero on a mismatch.
   python tools/bench_mvcc_maint.py [--keys 1e8] [--sizes 1024,65536,4194304] [--reps 5] [--arena-gb 0] [--out profiles/mvcc_maint_ab.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mvcc_scan import HBM_BYTES_PER_MS, VLEN, entries_of, mmm, record_keys, visible  # noqa: E402
from bench_mvcc_write import COMMIT_TS, START_TS, Request, timed, txn_handles, written_values  # noqa: E402
import bench_mvcc_write as BW  # noqa: E402
from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import mvcc as M  # noqa: E402

LINES = []
FAILED = []
SAMPLE = 4096
VERSION_ARRAYS = ("keys", "key_offsets", "commit_ts", "start_ts", "types", "values", "value_offsets")


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def gc_survivors(cts, types, m, sp):
    """GC(sp) restated over entries in store order: a mask of the entries that stay — those above the safe point, and per key the first
    PUT-or-DELETE at or under it iff it is a PUT (visible() names exactly that entry)"""
    keep = cts > np.uint64(sp)
    k = visible(cts, types, m, sp)
    keep[k[k >= 0]] = True
    return keep


class Store:
    """the v3 store, writable; per key the host keeps the chain length m, and per entry commitTS and type (1e8 keys: 3e8 entries, 2.7 GB)"""

    def __init__(self, ctx, K):
        self.ctx, self.K = ctx, K
        step = 1 << 22
        parts = [entries_of("v3", lo, min(K, lo + step), -1, 0) for lo in range(0, K, step)]
        self.m = np.concatenate([p[3] for p in parts])
        self.cts = np.concatenate([p[1] for p in parts])
        self.types = np.concatenate([p[2] for p in parts])
        self.first = np.cumsum(self.m) - self.m
        n = self.n = int(self.cts.size)
        vlen = np.where(self.types == abi.MVCC_PUT, VLEN, 0).astype(np.int64)
        self.vb = int(vlen.sum())
        sizes = dict(keys=19 * n, key_offsets=(n + 1) * 8, commit_ts=n * 8, start_ts=n * 8, types=n, values=self.vb, value_offsets=(n + 1) * 8)
        d = self.dev = {k: ctx.alloc(v + 64) for k, v in sizes.items()}
        at = vat = 0
        for key, cts, types, m in parts:
            e = key.size
            vl = vlen[at:at + e]
            voff = vat + np.concatenate([[0], np.cumsum(vl)])
            ctx.h2d(d["keys"] + 19 * at, record_keys(key * 3))
            ctx.h2d(d["key_offsets"] + 8 * at, (at + np.arange(e + 1, dtype=np.int64)) * 19)
            ctx.h2d(d["commit_ts"] + 8 * at, cts)
            ctx.h2d(d["start_ts"] + 8 * at, cts - np.uint64(1))
            ctx.h2d(d["types"] + at, types)
            ctx.h2d(d["value_offsets"] + 8 * at, voff)
            puts = np.flatnonzero(types == abi.MVCC_PUT)
            vals = np.empty((puts.size, VLEN), dtype=np.uint8)  # value = the entry's index, then a pattern
            vals[:, :8] = (puts + at).astype("<u8").view(np.uint8).reshape(-1, 8)
            vals[:, 8:] = (np.arange(VLEN - 8, dtype=np.uint8) + 65)[None, :]
            ctx.h2d(d["values"] + vat, vals)
            at += e
            vat = int(voff[-1])
        del parts
        self.bytes = sum(sizes.values())
        t0 = time.perf_counter()
        self.ms = M.MvccStore.create_rw(ctx, {k: (d[k], sizes[k] if k in ("keys", "values") else (n + 1 if k.endswith("offsets") else n)) for k in sizes}, device=True)
        self.create_ms = (time.perf_counter() - t0) * 1e3
        for p in d.values():  # (create copies the arrays in)
            ctx.free(p)

    def free(self):
        self.ms.close()


def version_bytes(z):
    return z["key_bytes"] + z["value_bytes"] + z["n"] * (8 + 8 + 8 + 8 + 1) + 16


def sample_reads(ms, st, ordinals, ts, keep, label):
    """the keys of `ordinals` as point reads at ts: the pairs must be those of getValue over the entries `keep` leaves (a mask over
    the store's entries; None: all) — the value's first 8 bytes name the entry"""
    want = []
    for o in ordinals:
        lo, hi = int(st.first[o]), int(st.first[o] + st.m[o])
        for e in range(lo, hi):
            if keep is not None and not keep[e]:
                continue
            if st.types[e] == abi.MVCC_ROLLBACK or int(st.cts[e]) > ts:
                continue
            if st.types[e] == abi.MVCC_PUT:
                want.append(e)
            break
    keys = record_keys(np.asarray(ordinals, dtype=np.int64) * 3)
    q = len(ordinals)
    offs = np.empty(2 * q + 1, dtype=np.int64)
    offs[0::2] = np.arange(q + 1) * 19
    offs[1::2] = offs[2::2]
    p = ms.scan_packed(keys.reshape(-1), offs, np.full(q, abi.MVCC_POINT, dtype=np.uint32), ts)
    try:
        got = p.values.read(np.uint8, p.value_bytes).reshape(-1, VLEN)[:, :8].copy().view("<u8").reshape(-1) if p.n else np.zeros(0, dtype=np.uint64)
        ok = p.n == len(want) and np.array_equal(got.astype(np.int64), np.asarray(want, dtype=np.int64))
    finally:
        p.free()
    if not ok:
        FAILED.append(label)
    return ok


def yardsticks(ctx, nxt, reps):
    """(a) and (b) over the next store's exported device arrays -> (copy ms list, create ms list, version-array bytes)"""
    arrs, z = nxt.export_device()
    n = z["n"]
    sizes = {k: arrs[k].nbytes for k in VERSION_ARRAYS}
    dst = {k: ctx.alloc(v + 64) for k, v in sizes.items()}

    def copy():
        for k, v in sizes.items():
            if v:
                _lib.check(ctx.lib.tsq_copy_d2d(ctx.h, C.c_void_p(dst[k]), C.c_void_p(arrs[k].p), v), ctx.h)
        ctx.sync()
    cp = timed(copy, reps)
    for p in dst.values():
        ctx.free(p)
    data = {"keys": (arrs["keys"].p, z["key_bytes"]), "key_offsets": (arrs["key_offsets"].p, n + 1), "commit_ts": (arrs["commit_ts"].p, n), "types": (arrs["types"].p, n),
            "values": (arrs["values"].p, z["value_bytes"]), "value_offsets": (arrs["value_offsets"].p, n + 1)}
    cr = timed(lambda: M.MvccStore(ctx, data, device=True).close(), reps)
    for a in arrs.values():
        a.free()
    return cp, cr, sum(sizes.values())


def report(label, ctx, cur, call, check, reps, moved_cur):
    """call() -> the next store (a new one every time); check(next) -> bool"""
    whole, kern, mark, ok = [], [], [], []
    nxt = None
    for rep in range(reps + 1):
        if nxt is not None:
            nxt.close()
        t0 = time.perf_counter()
        nxt = call()
        t1 = time.perf_counter()
        assert nxt is not cur, label
        if rep:
            whole.append((t1 - t0) * 1e3)
            kern.append(cur.last_maint["kernel_ms"])
            mark.append(cur.last_maint["mark_ms"])
            ok.append(check(nxt))
    cp, cr, nbytes = yardsticks(ctx, nxt, min(reps, 3))
    nxt.close()
    w, k, mk = float(np.median(whole)), float(np.median(kern)), float(np.median(mark))
    say("%-22s | whole %s kernel_ms %8.3f = marks %7.3f + apply %8.3f | (a) copy of the survivors %8.3f ms: x %5.2f | (b) create %8.3f ms: x %5.2f | %4.1f %% of 8 TB/s "
        "on %.2f GB read + %.2f GB written | count and sampled reads %s" %
        (label, mmm(whole), k, mk, k - mk, float(np.median(cp)), w / float(np.median(cp)), float(np.median(cr)), w / float(np.median(cr)),
         100 * (moved_cur + nbytes) / (w * HBM_BYTES_PER_MS), moved_cur / 1e9, nbytes / 1e9, "as restated" if all(ok) else "WRONG"))
    return w, k, mk


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=float, default=1e8)
    ap.add_argument("--sizes", default="1024,65536,4194304")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--arena-gb", type=float, default=0, help="tsq_ctx_reserve this much HBM first: the stores of the run are carved from one slab, "
                    "which takes the allocator out of the whole-call times (what does not fit falls back to hipMalloc)")
    a = ap.parse_args()
    K, sizes = int(a.keys), [int(x) for x in a.sizes.split(",")]
    rng = np.random.default_rng(11)
    say("tools/bench_mvcc_maint.py --keys %g --sizes %s --reps %d --arena-gb %g" % (a.keys, a.sizes, a.reps, a.arena_gb))
    say("ms per whole call, median [min .. max]; kernel_ms / marks / apply: the result's device time, median; x: whole call / yardstick")
    say()
    with _lib.Context(0) as ctx:
        if a.arena_gb > 0:
            try:
                ctx.reserve(int(a.arena_gb * (1 << 30)))
            except _lib.TsqError as e:
                say("(no arena: %s)" % e)
        t0 = time.perf_counter()
        st = Store(ctx, K)
        base = st.ms
        z = base.sizes()
        cur_bytes = version_bytes(z)
        say("== store v3: %d keys, %d versions (%.2f per key), %.2f GB of version arrays; built and uploaded in %.1f s, tsq_mvcc_create_rw %.1f ms" %
            (K, st.n, st.n / K, cur_bytes / 1e9, time.perf_counter() - t0, st.create_ms))
        sample = np.sort(rng.choice(K, min(SAMPLE, K), replace=False))
        top = int(st.cts.max())
        med = int(np.median(st.cts))
        # ---- gc
        gcs = []
        for name, sp in (("gc above every version", top + 1000), ("gc at median commitTS %d" % med, med)):
            keep = gc_survivors(st.cts, st.types, st.m, sp)
            want_n = int(keep.sum())

            def check(nxt, keep=keep, want_n=want_n, sp=sp, name=name):
                ok = nxt.n == want_n
                if not ok:
                    FAILED.append(name + " (count)")
                return ok and sample_reads(nxt, st, sample, top + 1000, keep, name) and sample_reads(nxt, st, sample, sp, keep, name) and \
                    sample_reads(nxt, st, sample, sp, None, name)  # (a read at or above the safe point sees what it saw before the GC)
            gc_w, gc_k, gc_m = report(name, ctx, base, lambda sp=sp: base.gc(b"", b"", sp), check, a.reps, cur_bytes)
            gcs.append((name, gc_m, gc_k - gc_m))
            say("   %d of %d versions stay" % (want_n, st.n))
            del keep
        # ---- delete_range
        k0, k1 = K * 45 // 100, K * 55 // 100
        lo, hi = record_keys(np.array([3 * k0, 3 * k1], dtype=np.int64))
        gone = int(st.m[k0:k1].sum())
        keep = np.ones(st.n, dtype=bool)
        keep[int(st.first[k0]):int(st.first[k0]) + gone] = False
        mixed = np.sort(np.concatenate([sample[: SAMPLE // 2], rng.choice(np.arange(k0, k1), min(SAMPLE // 2, k1 - k0), replace=False)]))

        def check_dr(nxt):
            ok = nxt.n == st.n - gone
            if not ok:
                FAILED.append("delete_range (count)")
            return ok and sample_reads(nxt, st, np.unique(mixed), top + 1000, keep, "delete_range")
        report("delete_range of K / 10", ctx, base, lambda: base.delete_range(lo.tobytes(), hi.tobytes()), check_dr, a.reps, cur_bytes)
        del keep
        # ---- resolve_lock, scan_lock; the prewrite of the same store beside them
        tag = 2
        for q in sizes:
            if q > K:
                continue
            vals = written_values(q, tag)
            tag += 1
            rq = Request(ctx, txn_handles("existing", q, K), vals)
            pw, pk = [], []
            locked = None
            for rep in range(a.reps + 1):
                if locked is not None:
                    locked.close()
                t0 = time.perf_counter()
                locked, _, _, r1 = base.write_packed("prewrite", rq.req, q)
                t1 = time.perf_counter()
                assert locked is not None and r1.locks_added == q
                if rep:
                    pw.append((t1 - t0) * 1e3)
                    pk.append(r1.kernel_ms)
            say("prewrite 2^%-2d (the write path on the same store) | whole %s kernel_ms %8.3f" % (int(np.log2(q)), mmm(pw), float(np.median(pk))))

            def check_rs(nxt, rq=rq, vals=vals, q=q):
                ok = nxt.n == st.n + q and nxt.n_locks == 0
                if not ok:
                    FAILED.append("resolve_lock 2^%d (count)" % int(np.log2(q)))
                if ok and not BW.verify(nxt, rq, vals, "resolve_lock 2^%d" % int(np.log2(q))):
                    FAILED.append("resolve_lock 2^%d (the committed values)" % int(np.log2(q)))
                    ok = False
                return ok and sample_reads(nxt, st, sample, START_TS - 1, None, "resolve_lock (older reads)")
            rs_w, rs_k, rs_m = report("resolve_lock 2^%-2d" % int(np.log2(q)), ctx, locked, lambda: locked.resolve_lock(b"", b"", START_TS, COMMIT_TS), check_rs, a.reps,
                                      cur_bytes)
            say("   marks / apply = %.3f; resolve_lock / prewrite = %.2f" % (rs_m / max(rs_k - rs_m, 1e-9), rs_w / float(np.median(pw))))
            if q == max(s for s in sizes if s <= K):
                sl, ok = [], True
                for rep in range(a.reps + 1):
                    t0 = time.perf_counter()
                    out = locked.scan_lock_packed(b"", b"", START_TS, device=True)
                    t1 = time.perf_counter()
                    if rep:
                        sl.append((t1 - t0) * 1e3)
                    n = out[0]
                    first_key = out[1].read(np.uint8, 19)
                    sts = out[5].read(np.uint64, n)
                    idx = out[6].read(np.int64, n)
                    ok = ok and n == q and np.array_equal(first_key, rq.keys_host[0]) and (sts == START_TS).all() and np.array_equal(idx, np.arange(q)) and \
                        locked.scan_lock_packed(b"", b"", START_TS - 1)[0] == 0
                    for d in out[1:]:
                        d.free()
                if not ok:
                    FAILED.append("scan_lock")
                moved = q * (19 + 19 + 8 + 8 + 8 + 16) * 2
                say("scan_lock over 2^%-2d locks | whole %s kernel_ms %8.3f | %4.1f %% of 8 TB/s on the locks' cells read and written | count, order and start_ts %s" %
                    (int(np.log2(q)), mmm(sl), locked.last_scan_lock["kernel_ms"], 100 * moved / (float(np.median(sl)) * HBM_BYTES_PER_MS), "as restated" if ok else "WRONG"))
            locked.close()
            rq.free()
        say()
        for name, mk, ap_ms in gcs:
            say("the marking passes together against the apply they feed, %s: marks %.3f ms, apply %.3f ms — the marks are %s" %
                (name, mk, ap_ms, "the smaller part" if mk < ap_ms else "NOT the smaller part"))
        st.free()
    if FAILED:
        say("FAILED: %s" % ", ".join(sorted(set(FAILED))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(1 if FAILED else 0)


if __name__ == "__main__":
    main()
