#!/usr/bin/env python3
"""The transaction buffer on device-resident streams: tsq_membuf_push + tsq_membuf_finish (csrc/tsq_membuf.hip), whole calls, beside
four yardsticks from the same run:
  (a) tsq_copy_d2d of the finished request's bytes (keys, values, two offset arrays, ops): the floor;
  (b) tsq_sort_* over the same keys as ONE TSQ_BYTES ORDER BY item with the value as payload: the route the project had before;
  (c) for record keys, tsq_sort_* on the decoded handle column (BIGINT) with the value as payload;
  (d) the host path of MvccStore._write — last-wins in a dict, sorted(), packing — on --host-keys keys, one core.
Shapes (per --keys N): `shuffled` — N record keys (19 bytes) of shuffled handles with 38-byte values, through the fixed-length form;
`ascending` — the same keys in order (no sort pass may run); `dup10` — N record keys of which a tenth are written twice; and, for the
first N only, `indexed` — N rows x (record key + a BIGINT index key of 37 bytes with the handle in it + a unique 8-byte-string index
key of 38 bytes whose value is the handle) in one buffer, record stream first.
Each is timed as push (all streams) and finish: host clock around calls that end in a device synchronise, median [min .. max] of
--reps after a warm-up, with the result's kernel_ms and sort_passes.  After every timed finish the entry count must equal the number
of distinct keys and 4096 sampled Gets must answer the key's rank (record keys) or a hit (index keys), 64 absent keys a miss; the
tool exits non-zero otherwise.
   python tools/bench_membuf.py [--keys 1e7,1e8] [--host-keys 1e6] [--reps 5] [--out profiles/membuf_ab.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))
sys.path.insert(0, os.path.dirname(os.path.abspath(__file__)))

from bench_mvcc_scan import HBM_BYTES_PER_MS, SIGN, TID, VLEN, mmm, record_keys  # noqa: E402
from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import kv  # noqa: E402
from tinysql_amd.dupcheck import DevArray  # noqa: E402
from tinysql_amd.gpu_pipeline import DeviceColumn  # noqa: E402

LINES, FAILED = [], []


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def be8(v):
    return (v.astype(np.uint64) ^ SIGN).astype(">u8").view(np.uint8).reshape(-1, 8)


def index_prefix(ix, n):
    out = np.empty((n, 19), dtype=np.uint8)
    out[:, 0] = ord("t")
    out[:, 1:9] = np.frombuffer((np.uint64(TID) ^ SIGN).astype(">u8").tobytes(), dtype=np.uint8)
    out[:, 9], out[:, 10] = ord("_"), ord("i")
    out[:, 11:] = np.frombuffer((np.uint64(ix) ^ SIGN).astype(">u8").tobytes(), dtype=np.uint8)
    return out


def int_index_keys(handles):
    """t{tid}_i{1} + intFlag + a (= handle mod 1000) + intFlag + handle: 37 bytes"""
    n = handles.size
    out = np.empty((n, 37), dtype=np.uint8)
    out[:, :19] = index_prefix(1, n)
    out[:, 19], out[:, 28] = 3, 3
    out[:, 20:28] = be8(handles % 1000)
    out[:, 29:] = be8(handles)
    return out


def str_index_keys(handles):
    """t{tid}_i{2} + bytesFlag + an 8-byte string unique per handle in memcomparable form (its group, 0xFF, a padding group, 0xF7): 38 bytes"""
    n = handles.size
    out = np.zeros((n, 38), dtype=np.uint8)
    out[:, :19] = index_prefix(2, n)
    out[:, 19] = 1
    out[:, 20:28] = (handles.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)).astype(">u8").view(np.uint8).reshape(-1, 8)  # (an odd multiplier: a bijection of the handles)
    out[:, 28], out[:, 37] = 0xFF, 0xF7
    return out


def values_for(handles):
    vals = np.empty((handles.size, VLEN), dtype=np.uint8)
    vals[:, :8] = handles.astype("<i8").view(np.uint8).reshape(-1, 8)
    vals[:, 8:] = (np.arange(VLEN - 8, dtype=np.uint8) + 97)[None, :]
    return vals


class Stream:
    """one stream of Sets in HBM: keys of one length (pushed through the fixed-length form), values of one length with their offsets"""

    def __init__(self, ctx, keys, vals):
        self.n, self.klen, self.vlen = keys.shape[0], keys.shape[1], vals.shape[1]
        self.keys, self.vals = DevArray(ctx, keys.reshape(-1)), DevArray(ctx, vals.reshape(-1))
        self.voff = DevArray(ctx, np.arange(self.n + 1, dtype=np.int64) * self.vlen)
        self.koff = DevArray(ctx, np.arange(self.n + 1, dtype=np.int64) * self.klen)  # (for the sort yardstick; the push passes none)

    def push(self, mb):
        mb.set_packed(self.keys.p, None, self.n * self.klen, self.n, self.vals.p, self.voff.p, self.n * self.vlen, device=True)

    def free(self):
        for a in (self.keys, self.vals, self.voff, self.koff):
            a.free()


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def sort_yardstick(ctx, key_col, key_type, st, reps):
    """tsq_sort_* over (key, value) with the key as the one ORDER BY item: create, push, finish, pull into sized buffers, destroy"""
    lib, n = ctx.lib, st.n
    cfg = abi.SortCfg()
    cfg.n_cols, cfg.n_keys, cfg.limit_offset, cfg.limit_count, cfg.max_chunk_size = 2, 1, 0, -1, 1024
    cfg.col_types[0], cfg.col_types[1], cfg.key_col[0], cfg.key_desc[0] = key_type, abi.BYTES, 0, 0
    val_col = DeviceColumn(ctx, abi.BYTES, n, data=st.vals.p, offsets=st.voff.p, cap_bytes=n * st.vlen)
    out = [DeviceColumn(ctx, key_type, n, cap_bytes=n * st.klen), DeviceColumn(ctx, abi.BYTES, n, cap_bytes=n * st.vlen)]

    def run():
        h = C.c_void_p()
        _lib.check(lib.tsq_sort_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
        try:
            cols = (abi.Col * 2)(key_col.col(n), val_col.col(n))
            _lib.check(lib.tsq_sort_push(h, cols, 2, n), h)
            _lib.check(lib.tsq_sort_finish(h), h)
            oc = (abi.Col * 2)(out[0].col(n), out[1].col(n))
            got, eos = C.c_int64(0), C.c_int32(0)
            _lib.check(lib.tsq_sort_pull(h, oc, 2, n, C.byref(got), C.byref(eos)), h)
            assert got.value == n, got.value
        finally:
            lib.tsq_sort_destroy(h)
        ctx.sync()
    try:
        return timed(run, reps)
    finally:
        for c in out:
            c.free()


def copy_floor(ctx, req, reps):
    parts = [(req.keys, req.key_bytes), (req.key_offsets, (req.n_keys + 1) * 8), (req.ops, req.n_keys), (req.values, req.value_bytes), (req.value_offsets, (req.n_keys + 1) * 8)]
    dst = [ctx.alloc(b + 64) for _, b in parts]

    def run():
        for d, (p, b) in zip(dst, parts):
            if b:
                _lib.check(ctx.lib.tsq_copy_d2d(ctx.h, C.c_void_p(d), C.c_void_p(p), b), ctx.h)
        ctx.sync()
    try:
        return timed(run, reps), sum(b for _, b in parts)
    finally:
        for d in dst:
            ctx.free(d)


def check(mb, res, label, n_distinct, hs, rec_base, other_keys, rng):
    """the entry count; sampled Gets of record keys (hs: the distinct handles ascending; index = rec_base + the handle's rank), of other keys (a hit) and of absent keys"""
    ok = res["n_entries"] == n_distinct
    pick = hs[rng.integers(0, hs.size, 4096)]
    got = mb.get_packed(record_keys(pick).reshape(-1), None, 19 * pick.size, pick.size)
    ok = ok and np.array_equal(got, rec_base + np.searchsorted(hs, pick))
    absent = record_keys(np.arange(64, dtype=np.int64) + int(hs[-1]) + 1)
    ok = ok and (mb.get_packed(absent.reshape(-1), None, 19 * 64, 64) == -1).all()
    for keys in other_keys:
        rows = keys[rng.integers(0, keys.shape[0], 1024)]
        g = mb.get_packed(np.ascontiguousarray(rows).reshape(-1), None, rows.size, rows.shape[0])
        ok = ok and (g >= 0).all() and (g < rec_base).all()
    if not ok:
        FAILED.append(label)
    return ok


def run_shape(ctx, label, streams, n_distinct, rec_handles, rec_base, other_keys, reps, handle_sort=True):
    rng = np.random.default_rng(5)
    distinct = np.unique(rec_handles)
    push_ms, fin_ms, kern, passes, checks = [], [], [], [], []
    floor = moved = None
    for rep in range(reps + 1):
        with kv.MemBuffer(ctx) as mb:
            ctx.sync()
            t0 = time.perf_counter()
            for st in streams:
                st.push(mb)
            ctx.sync()
            t1 = time.perf_counter()
            res = mb.finish()
            t2 = time.perf_counter()
            if rep:  # (the first is the warm-up)
                push_ms.append((t1 - t0) * 1e3)
                fin_ms.append((t2 - t1) * 1e3)
                kern.append(res["kernel_ms"])
                passes.append(res["sort_passes"])
                checks.append(check(mb, res, label, n_distinct, distinct, rec_base, other_keys, rng))
            if rep == reps:
                floor, req_bytes = copy_floor(ctx, mb.request(), reps)
                pushed = sum(s.n * (s.klen + s.vlen + 8) for s in streams)
                moved = pushed + req_bytes  # read what was pushed once, write the request once
    f, fl = float(np.median(fin_ms)), float(np.median(floor))
    say("%-22s | push %s | finish %s kernel_ms %9.3f passes %2d | (a) copy %s | finish / (a) %6.2f | %5.2f %% of 8 TB/s | count and sampled Gets %s" %
        (label, mmm(push_ms), mmm(fin_ms), float(np.median(kern)), int(np.median(passes)), mmm(floor), f / fl, 100 * moved / (f * HBM_BYTES_PER_MS),
         "right" if all(checks) else "WRONG"))
    for st in streams:
        key_col = DeviceColumn(ctx, abi.BYTES, st.n, data=st.keys.p, offsets=st.koff.p, cap_bytes=st.n * st.klen)
        b = sort_yardstick(ctx, key_col, abi.BYTES, st, reps)
        say("%-22s |   (b) tsq_sort_* on the %d-byte keys as one TSQ_BYTES item, %d-byte value as payload: %s | finish / (b) %6.2f%s" %
            ("", st.klen, st.vlen, mmm(b), f / float(np.median(b)), "  (one stream of %d; the buffer sorts all streams together)" % len(streams) if len(streams) > 1 else ""))
    if handle_sort:
        st = streams[0]
        hcol_arr = DevArray(ctx, np.ascontiguousarray(rec_handles[:st.n], dtype=np.int64))
        try:
            c = sort_yardstick(ctx, DeviceColumn(ctx, abi.I64, st.n, data=hcol_arr.p), abi.I64, st, reps)
        finally:
            hcol_arr.free()
        say("%-22s |   (c) tsq_sort_* on the decoded handles (BIGINT), %d-byte value as payload: %s | finish / (c) %6.2f" % ("", st.vlen, mmm(c), f / float(np.median(c))))
    return f


def host_yardstick(n):
    """(d) the lines of MvccStore._write in front of the device call: the last write of every key in a dict, sorted(), the packing"""
    rng = np.random.default_rng(9)
    hs = rng.permutation(n).astype(np.int64)
    keys = [bytes(k) for k in record_keys(hs)]
    vals = [bytes(v) for v in values_for(hs)]
    t0 = time.perf_counter()
    last = {}
    for i, k in enumerate(keys):
        last[k] = i
    order = sorted(last.values(), key=lambda i: keys[i])
    kb = b"".join(keys[i] for i in order)
    vb = b"".join(vals[i] for i in order)
    ko = np.cumsum([0] + [len(keys[i]) for i in order])
    vo = np.cumsum([0] + [len(vals[i]) for i in order])
    ms = (time.perf_counter() - t0) * 1e3
    assert len(kb) == 19 * n and len(vb) == VLEN * n and ko[-1] == 19 * n and vo[-1] == VLEN * n
    say("(d) the host path of MvccStore._write (dict, sorted, packing) on %d shuffled record keys, one core: %.1f ms = %.3g keys/s" % (n, ms, n / ms * 1e3))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", default="1e7,1e8")
    ap.add_argument("--host-keys", type=float, default=1e6)
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--no-host", action="store_true", help="leave yardstick (d) out")
    a = ap.parse_args()
    sizes = [int(float(x)) for x in a.keys.split(",")]
    say("tools/bench_membuf.py --keys %s --host-keys %g --reps %d" % (a.keys, a.host_keys, a.reps))
    say("ms per whole call, median [min .. max]; kernel_ms: the result's stream time, median; the % column: (pushed bytes read + request bytes written) / finish time, against 8 TB/s")
    say()
    with _lib.Context(0) as ctx:
        for si, n in enumerate(sizes):
            rng = np.random.default_rng(3)
            hs = rng.permutation(n).astype(np.int64) * 3 - n  # distinct, both signs
            say("== %d record keys, %d-byte values" % (n, VLEN))
            st = Stream(ctx, record_keys(hs), values_for(hs))
            run_shape(ctx, "shuffled   N=%.0e" % n, [st], n, hs, 0, [], a.reps)
            st.free()
            asc = np.sort(hs)
            st = Stream(ctx, record_keys(asc), values_for(asc))
            run_shape(ctx, "ascending  N=%.0e" % n, [st], n, asc, 0, [], a.reps)
            st.free()
            dup = np.concatenate([hs[: n - n // 10], hs[rng.integers(0, n - n // 10, n // 10)]])
            st = Stream(ctx, record_keys(dup), values_for(dup))
            run_shape(ctx, "dup10      N=%.0e" % n, [st], n - n // 10, dup, 0, [], a.reps)
            st.free()
            if si == 0:
                ik, sk = int_index_keys(hs), str_index_keys(hs)
                streams = [Stream(ctx, record_keys(hs), values_for(hs)), Stream(ctx, ik, np.full((n, 1), ord("0"), dtype=np.uint8)),
                           Stream(ctx, sk, np.ascontiguousarray(be8(hs)))]
                run_shape(ctx, "indexed    N=%.0e x3" % n, streams, 3 * n, hs, 2 * n, [ik, sk], a.reps)  # ("_i" sorts under "_r": both indexes come first)
                for s in streams:
                    s.free()
            say()
    if not a.no_host:
        host_yardstick(int(a.host_keys))
    if FAILED:
        say("FAILED: a wrong entry count or sampled Get: %s" % ", ".join(sorted(set(FAILED))))
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "w") as f:
            f.write("\n".join(LINES) + "\n")
    sys.exit(1 if FAILED else 0)


if __name__ == "__main__":
    main()
