#!/usr/bin/env python3
"""MVCC writes on a device-resident store: tsq_mvcc_prewrite + tsq_mvcc_commit into the next store (csrc/tsq_mvcc_write.hip), whole
calls, beside three yardsticks from the same run:
  (a) tsq_copy_d2d of the store's version arrays (keys, offsets, commitTS, startTS, types, values): what a full rewrite must move
      at least;
  (b) tsq_mvcc_create from the next store's exported device arrays: the rebuild (head flags, ordinals, universe) every apply contains;
  (c) the sequential model of tests/mvcc_ref.py on one host core, at --host-keys keys.
The store: --keys record keys (19 bytes, handles 0, 3, 6, ..) with one 38-byte version each — the v1 store of tools/bench_mvcc_scan.py.
Transactions of --sizes Puts (38-byte values) in three shapes: `new` — keys the store does not hold, interleaved with its keys
(handles 3 k + 1, spread over the whole store); `existing` — keys of the store, spread likewise; `append` — all behind the last key.
Each is timed as prewrite (into store 1) and commit (store 1 into store 2): host clock around calls that end in a device
synchronise, median [min .. max] of --reps after a warm-up, and the result's kernel_ms.  After every timed commit the written keys
are read as points from store 2 at commitTS — every pair must come back with its written value — and at commitTS - 1 — no written
value may come back; the tool exits non-zero otherwise.
   python tools/bench_mvcc_write.py [--keys 1e8] [--sizes 1024,65536,4194304] [--reps 5] [--out profiles/mvcc_write_ab.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mvcc_scan import HBM_BYTES_PER_MS, VLEN, mmm, record_keys  # noqa: E402
from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import mvcc as M  # noqa: E402
from tinysql_amd.dupcheck import DevArray  # noqa: E402

LINES = []
BASE_CTS, START_TS, COMMIT_TS = 16, 1000, 1001
FAILED = []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def build_store(ctx, K):
    """K keys, one put each at commitTS 16 (startTS 15); built on the host in slices and uploaded; -> (MvccStore, the device arrays)"""
    names = dict(keys=19 * K, key_offsets=(K + 1) * 8, commit_ts=K * 8, start_ts=K * 8, types=K, values=VLEN * K, value_offsets=(K + 1) * 8)
    d = {k: ctx.alloc(v + 64) for k, v in names.items()}
    step = 1 << 22
    tail = (np.arange(VLEN - 8, dtype=np.uint8) + 65)[None, :]
    for lo in range(0, K, step):
        hi = min(K, lo + step)
        k = np.arange(lo, hi, dtype=np.int64)
        ctx.h2d(d["keys"] + 19 * lo, record_keys(k * 3))
        ctx.h2d(d["key_offsets"] + 8 * lo, (lo + np.arange(hi - lo + 1, dtype=np.int64)) * 19)
        ctx.h2d(d["commit_ts"] + 8 * lo, np.full(hi - lo, BASE_CTS, dtype=np.uint64))
        ctx.h2d(d["start_ts"] + 8 * lo, np.full(hi - lo, BASE_CTS - 1, dtype=np.uint64))
        ctx.h2d(d["types"] + lo, np.zeros(hi - lo, dtype=np.uint8))
        ctx.h2d(d["value_offsets"] + 8 * lo, (lo + np.arange(hi - lo + 1, dtype=np.int64)) * VLEN)
        vals = np.empty((hi - lo, VLEN), dtype=np.uint8)
        vals[:, :8] = k.astype("<u8").view(np.uint8).reshape(-1, 8)
        vals[:, 8:] = tail
        ctx.h2d(d["values"] + VLEN * lo, vals)
    t0 = time.perf_counter()
    ms = M.MvccStore.create_rw(ctx, {"keys": (d["keys"], 19 * K), "key_offsets": (d["key_offsets"], K + 1), "commit_ts": (d["commit_ts"], K), "start_ts": (d["start_ts"], K),
                                     "types": (d["types"], K), "values": (d["values"], VLEN * K), "value_offsets": (d["value_offsets"], K + 1)}, device=True)
    return ms, d, names, (time.perf_counter() - t0) * 1e3


def txn_handles(shape, q, K):
    if shape == "append":
        return 3 * K + np.arange(q, dtype=np.int64)
    at = (np.arange(q, dtype=np.int64) * K) // q  # q distinct key ordinals spread over the store (q <= K)
    return at * 3 + (1 if shape == "new" else 0)


def written_values(q, tag):
    vals = np.empty((q, VLEN), dtype=np.uint8)
    vals[:, :8] = (np.arange(q, dtype=np.int64) | (tag << 40)).astype("<u8").view(np.uint8).reshape(-1, 8)
    vals[:, 8:] = (np.arange(VLEN - 8, dtype=np.uint8) + 97)[None, :]
    return vals


class Request:
    """one transaction's Puts, device resident"""

    def __init__(self, ctx, handles, vals):
        q = handles.size
        self.q, self.keys_host = q, record_keys(handles)
        self.arrs = [DevArray(ctx, self.keys_host), DevArray(ctx, np.arange(q + 1, dtype=np.int64) * 19), DevArray(ctx, np.zeros(q, dtype=np.uint8)), DevArray(ctx, vals),
                     DevArray(ctx, np.arange(q + 1, dtype=np.int64) * VLEN)]
        self.primary = self.keys_host[0].copy()
        r = self.req = abi.MvccWriteReq()
        r.keys, r.key_offsets, r.key_bytes, r.n_keys = self.arrs[0].p, self.arrs[1].p, 19 * q, q
        r.ops, r.values, r.value_offsets, r.value_bytes = self.arrs[2].p, self.arrs[3].p, self.arrs[4].p, VLEN * q
        r.primary, r.primary_len = self.primary.ctypes.data, 19
        r.start_ts, r.commit_ts, r.ttl, r.flags = START_TS, COMMIT_TS, 3000, abi.COL_DEVICE

    def free(self):
        for a in self.arrs:
            a.free()


def read_points(ms, rq, ts):
    """the written keys as point reads at ts -> the values of the pairs that came back, [n, 38] (every value here has 38 bytes)"""
    offs = np.empty(2 * rq.q + 1, dtype=np.int64)
    offs[0::2] = np.arange(rq.q + 1) * 19
    offs[1::2] = offs[2::2]
    p = ms.scan_packed(rq.keys_host.reshape(-1), offs, np.full(rq.q, abi.MVCC_POINT, dtype=np.uint32), ts)
    try:
        assert p.value_bytes == VLEN * p.n
        return p.values.read(np.uint8, p.value_bytes).reshape(-1, VLEN), p.n
    finally:
        p.free()


def verify(store2, rq, vals, label):
    got, n = read_points(store2, rq, COMMIT_TS)
    ok_at = n == rq.q and np.array_equal(got, vals)
    got, n = read_points(store2, rq, COMMIT_TS - 1)
    ok_before = not (n and (got[:, 8] == 97).any())  # (a written value starts its pattern at 'a', a value of the store at 'A')
    if not (ok_at and ok_before):
        FAILED.append(label)
    return ok_at and ok_before


def run_case(ctx, base, shape, q, K, reps, tag, floor_ms, create_ms, moved):
    handles = txn_handles(shape, q, K)
    vals = written_values(q, tag)
    rq = Request(ctx, handles, vals)
    label = "%-8s 2^%-2d" % (shape, int(np.log2(q)))
    pw, cm, pk, ck, checks = [], [], [], [], []
    try:
        for rep in range(reps + 1):
            t0 = time.perf_counter()
            s1, _, _, r1 = base.write_packed("prewrite", rq.req, q)
            t1 = time.perf_counter()
            assert s1 is not None and r1.locks_added == q, (label, r1.n_errors, r1.first_error)
            s2, _, _, r2 = s1.write_packed("commit", rq.req, q)
            t2 = time.perf_counter()
            assert s2 is not None and r2.versions_added == q and r2.locks_removed == q and r2.versions_replaced == 0, label
            if rep:  # (the first is the warm-up)
                pw.append((t1 - t0) * 1e3)
                cm.append((t2 - t1) * 1e3)
                pk.append(r1.kernel_ms)
                ck.append(r2.kernel_ms)
                checks.append(verify(s2, rq, vals, label))
            s1.close()
            s2.close()
    finally:
        rq.free()
    c = float(np.median(cm))
    say("%s | prewrite %s kernel_ms %8.3f | commit %s kernel_ms %8.3f | commit / (a) %5.2f | commit / (b) %5.2f | %5.1f %% of 8 TB/s | reads after every commit %s" %
        (label, mmm(pw), float(np.median(pk)), mmm(cm), float(np.median(ck)), c / floor_ms, c / create_ms, 100 * moved / (c * HBM_BYTES_PER_MS),
         "as written" if all(checks) else "WRONG"))


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def copy_floor(ctx, d, names, reps):
    dst = {k: ctx.alloc(v + 64) for k, v in names.items()}

    def run():
        for k, v in names.items():
            _lib.check(ctx.lib.tsq_copy_d2d(ctx.h, C.c_void_p(dst[k]), C.c_void_p(d[k]), v), ctx.h)
        ctx.sync()
    t = timed(run, reps)
    for p in dst.values():
        ctx.free(p)
    return t


def create_yardstick(ctx, base, K, reps):
    """(b): the next store of a 2^16 `new` transaction, exported, and tsq_mvcc_create over the exported device arrays"""
    q = min(1 << 16, K)
    rq = Request(ctx, txn_handles("new", q, K), written_values(q, 1))
    s1, _, _, _ = base.write_packed("prewrite", rq.req, q)
    s2, _, _, _ = s1.write_packed("commit", rq.req, q)
    s1.close()
    arrs, z = s2.export_device()
    s2.close()
    rq.free()
    n = z["n"]
    data = {"keys": (arrs["keys"].p, z["key_bytes"]), "key_offsets": (arrs["key_offsets"].p, n + 1), "commit_ts": (arrs["commit_ts"].p, n), "types": (arrs["types"].p, n),
            "values": (arrs["values"].p, z["value_bytes"]), "value_offsets": (arrs["value_offsets"].p, n + 1)}

    def run():
        M.MvccStore(ctx, data, device=True).close()
    t = timed(run, reps)
    for a in arrs.values():
        a.free()
    return t


def host_yardstick(n, sizes):
    from tests import mvcc_ref as R
    say("== (c) the sequential model of tests/mvcc_ref.py on one host core, a store of %d keys with one version each" % n)
    keys = [bytes(k) for k in record_keys(np.arange(n, dtype=np.int64) * 3)]
    s = R.Store()
    for k in keys:
        s.versions[k] = [R.Value(R.PUT, BASE_CTS - 1, BASE_CTS, b"v" * VLEN)]
    for q in sizes:
        if q > n:
            continue
        new = [bytes(k) for k in record_keys(txn_handles("new", q, n))]
        t0 = time.perf_counter()
        s.prewrite([(R.OP_PUT, k, b"w" * VLEN) for k in new], new[0], START_TS + q)
        t1 = time.perf_counter()
        s.commit(new, START_TS + q, COMMIT_TS + q)
        t2 = time.perf_counter()
        say("new      2^%-2d | prewrite %9.3f ms | commit %9.3f ms   (dict updates; no array is rewritten)" % (int(np.log2(q)), (t1 - t0) * 1e3, (t2 - t1) * 1e3))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=float, default=1e8)
    ap.add_argument("--host-keys", type=float, default=1e6)
    ap.add_argument("--sizes", default="1024,65536,4194304")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-host", action="store_true", help="leave yardstick (c) out")
    a = ap.parse_args()
    K, sizes = int(a.keys), [int(x) for x in a.sizes.split(",")]
    say("tools/bench_mvcc_write.py --keys %g --host-keys %g --sizes %s --reps %d" % (a.keys, a.host_keys, a.sizes, a.reps))
    say("ms per whole call, median [min .. max]; kernel_ms: the result's device time, median")
    say()
    with _lib.Context(0) as ctx:
        t0 = time.perf_counter()
        base, d, names, create_rw_ms = build_store(ctx, K)
        z = base.sizes()
        arrays = z["key_bytes"] + z["value_bytes"] + z["n"] * (8 + 8 + 8 + 8 + 1)
        say("== store: %d keys, one version each, %.2f GB of version arrays (keys, values, two offset arrays, commitTS, startTS, types); built and uploaded in %.1f s, "
            "tsq_mvcc_create_rw %.1f ms" % (K, arrays / 1e9, time.perf_counter() - t0, create_rw_ms))
        fl = copy_floor(ctx, d, names, a.reps)
        say("(a) tsq_copy_d2d of the version arrays: %s ms  (%.1f %% of 8 TB/s on read + write)" % (mmm(fl), 100 * 2 * arrays / (np.median(fl) * HBM_BYTES_PER_MS)))
        cr = create_yardstick(ctx, base, K, a.reps)
        say("(b) tsq_mvcc_create from the exported device arrays of a next store (the copy-in and the index build): %s ms" % mmm(cr))
        say("the %% column: (version arrays of the current store read + of the next store written) / commit time, against 8 TB/s")
        say()
        tag = 2
        for q in sizes:
            if q > K:
                continue
            for shape in ("new", "existing", "append"):
                run_case(ctx, base, shape, q, K, a.reps, tag, float(np.median(fl)), float(np.median(cr)), 2 * arrays + q * (19 + VLEN + 25))
                tag += 1
        say()
        base.close()
        for p in d.values():
            ctx.free(p)
    if not a.no_host:
        host_yardstick(int(a.host_keys), sizes)
    if FAILED:
        say("FAILED: the reads after a commit did not return what was written: %s" % ", ".join(sorted(set(FAILED))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(1 if FAILED else 0)


if __name__ == "__main__":
    main()
