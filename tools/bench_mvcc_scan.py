#!/usr/bin/env python3
"""MVCC snapshot reads on a device-resident store: tsq_mvcc_scan + tsq_mvcc_fetch (csrc/tsq_mvcc.hip), whole calls, beside three
yardsticks from the same run:
  (a) tsq_rows_gather alone over the same visible rows (their entry indices computed here): the copy floor — the scan cannot beat it;
  (b) the share of the 8 TB/s roofline on the bytes that must move: 9 bytes per entry examined (commitTS + type), one read of the
      chosen keys and values and one write of them;
  (c) the numpy restatement of the read on one host core, at --host-keys keys.

Stores (--stores, comma separated), --keys record keys (19 bytes) with 38-byte values, built on the host and uploaded:
  v1     exactly one version per key
  v1.2   1 + (every fifth key a second version)                     (mean 1.2)
  v3     1..5 versions per key (mean 3), 5 % deletes, 1 % rollbacks
  hot    v1 plus one key in the middle with --hot versions (default 1e6), the newer half of them rollbacks
Reads, each timed as scan / fetch / both (host clock around calls that end in a device synchronise; median [min .. max] of --reps
windows after a warm-up): one full range ascending and descending; 2^10 ranges; 2^20 point reads, hit and miss mixed; limit 1.
Every read's pairs are compared row by row with the numpy restatement (key bytes, value bytes, both offset arrays: "rows identical");
the full ascending read also byte for byte with yardstick (a)'s output.  --chains: the A/B of TSQ_KNOB_MVCC_WAVE_CHAIN on the stores named.
   python tools/bench_mvcc_scan.py [--keys 1e8] [--stores v1,v1.2,v3,hot] [--reps 5] [--out profiles/mvcc_scan_ab.txt]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import mvcc as M  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3
VLEN = 38
SIGN = np.uint64(1 << 63)
TID = 41
LINES = []
READ_TS = 1 << 40  # above every commitTS of the generated stores: a read sees the newest version that is not a rollback


def say(s=""):
    print(s, flush=True)
    LINES.append(s)


def mmm(v):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))


def record_keys(handles):
    out = np.empty((handles.size, 19), dtype=np.uint8)
    out[:, 0] = ord("t")
    out[:, 1:9] = np.frombuffer((np.uint64(TID) ^ SIGN).astype(">u8").tobytes(), dtype=np.uint8)
    out[:, 9], out[:, 10] = ord("_"), ord("r")
    out[:, 11:] = (handles.astype(np.uint64) ^ SIGN).astype(">u8").view(np.uint8).reshape(-1, 8)
    return out


def chain_lengths(kind, lo, hi, hot_at, hot):
    k = np.arange(lo, hi, dtype=np.int64)
    if kind == "v1.2":
        m = 1 + (k % 5 == 0)
    elif kind == "v3":
        m = 1 + (k * 2654435761 >> 7) % 5
    else:
        m = np.ones(hi - lo, dtype=np.int64)
    m = m.astype(np.int64)
    if kind == "hot" and lo <= hot_at < hi:
        m[hot_at - lo] = hot
    return m


def entries_of(kind, lo, hi, hot_at, hot):
    """the versions of keys [lo, hi): per entry (key ordinal, commitTS, type); versions of a key in descending commitTS"""
    m = chain_lengths(kind, lo, hi, hot_at, hot)
    key = np.repeat(np.arange(lo, hi, dtype=np.int64), m)
    first = np.cumsum(m) - m
    j = np.arange(key.size, dtype=np.int64) - np.repeat(first, m)  # 0 = the newest
    cts = (np.repeat(m, m) - j) * 16 + (key & 7)
    types = np.zeros(key.size, dtype=np.uint8)
    if kind == "v3":
        h = (key * 40503 + j * 9973) % 100
        types[h < 5] = abi.MVCC_DELETE
        types[h == 5] = abi.MVCC_ROLLBACK
    if kind == "hot":  # the newer half of the hot key's chain is a run of rollbacks: what a read has to step over
        types[(key == hot_at) & (j < hot // 2)] = abi.MVCC_ROLLBACK
    return key, cts.astype(np.uint64), types, m


def visible(cts, types, m, ts):
    """the numpy restatement of getValue over entries in store order: per key the entry that decides (-1: none) — the first with
    commitTS <= ts that is not a rollback, if it is a put"""
    n = cts.size
    ok = (cts <= np.uint64(ts)) & (types != abi.MVCC_ROLLBACK)
    idx = np.where(ok, np.arange(n, dtype=np.int64), n)
    first = np.minimum.reduceat(idx, np.cumsum(m) - m)
    end = np.cumsum(m)
    hit = first < end
    out = np.where(hit, first, -1)
    out[hit & (types[np.minimum(first, n - 1)] != abi.MVCC_PUT)] = -1
    return out


class Store:
    def __init__(self, ctx, kind, n_keys, hot):
        self.ctx, self.kind, self.K = ctx, kind, n_keys
        hot_at = n_keys // 2
        step = 1 << 22
        counts = [int(chain_lengths(kind, lo, min(n_keys, lo + step), hot_at, hot).sum()) for lo in range(0, n_keys, step)]
        n = self.n = sum(counts)
        self.key_bytes = 19 * n
        d = {"keys": ctx.alloc(19 * n + 64), "key_offsets": ctx.alloc((n + 1) * 8 + 64), "commit_ts": ctx.alloc(n * 8 + 64), "types": ctx.alloc(n + 64),
             "value_offsets": ctx.alloc((n + 1) * 8 + 64)}
        at = vat = 0
        vis, chunks = [], []
        for lo in range(0, n_keys, step):
            hi = min(n_keys, lo + step)
            key, cts, types, m = entries_of(kind, lo, hi, hot_at, hot)
            vlen = np.where(types == abi.MVCC_PUT, VLEN, 0).astype(np.int64)
            voff = vat + np.concatenate([[0], np.cumsum(vlen)])
            chunks.append((at, types, int(voff[0])))
            ctx.h2d(d["keys"] + 19 * at, record_keys(key * 3))
            ctx.h2d(d["key_offsets"] + 8 * at, (at + np.arange(key.size + 1, dtype=np.int64)) * 19)
            ctx.h2d(d["commit_ts"] + 8 * at, cts)
            ctx.h2d(d["types"] + at, types)
            ctx.h2d(d["value_offsets"] + 8 * at, voff)
            v = visible(cts, types, m, READ_TS)
            vis.append(np.where(v >= 0, v + at, -1))
            at += key.size
            vat = int(voff[-1])
        self.value_bytes = vat
        d["values"] = ctx.alloc(vat + 64)
        for at0, types, v0 in chunks:  # value = the entry's index, then a pattern
            puts = np.flatnonzero(types == abi.MVCC_PUT)
            vals = np.empty((puts.size, VLEN), dtype=np.uint8)
            vals[:, :8] = (puts + at0).astype("<u8").view(np.uint8).reshape(-1, 8)
            vals[:, 8:] = (np.arange(VLEN - 8, dtype=np.uint8) + 65)[None, :]
            ctx.h2d(d["values"] + v0, vals)
        self.dev = d
        self.visible = np.concatenate(vis)  # per key
        self.rows = self.visible[self.visible >= 0]
        t0 = time.perf_counter()
        self.ms = M.MvccStore(ctx, {"keys": (d["keys"], 19 * n), "key_offsets": (d["key_offsets"], n + 1), "commit_ts": (d["commit_ts"], n), "types": (d["types"], n),
                                    "values": (d["values"], vat), "value_offsets": (d["value_offsets"], n + 1)}, device=True)
        self.create_ms = (time.perf_counter() - t0) * 1e3
        cap = self.cap = max(self.rows.size, 1 << 20)
        self.out = {"k": ctx.alloc(19 * cap + 64), "ko": ctx.alloc((cap + 1) * 8 + 64), "v": ctx.alloc(VLEN * cap + 64), "vo": ctx.alloc((cap + 1) * 8 + 64)}

    def free(self):
        self.ms.close()
        for p in list(self.dev.values()) + list(self.out.values()):
            self.ctx.free(p)


def timed(fn, reps):
    fn()
    out = []
    for _ in range(reps):
        t0 = time.perf_counter()
        fn()
        out.append((time.perf_counter() - t0) * 1e3)
    return out


def verify_rows(st, n_pairs, want_keys):
    """every fetched pair against the numpy restatement, row by row: pair i must be key ordinal want_keys[i] (its 19 key bytes) with
    the value of the entry the restatement chose for that key (its 38 bytes), and the two offset arrays must be i * 19 and i * 38"""
    ctx = st.ctx
    if n_pairs != want_keys.size:
        return False
    step = 1 << 23
    tail = np.arange(VLEN - 8, dtype=np.uint8) + 65
    for lo in range(0, n_pairs, step):
        n = min(step, n_pairs - lo)
        k, v = np.empty(19 * n, dtype=np.uint8), np.empty(VLEN * n, dtype=np.uint8)
        ko, vo = np.empty(n + 1, dtype=np.int64), np.empty(n + 1, dtype=np.int64)
        for h, d in ((k, st.out["k"] + 19 * lo), (v, st.out["v"] + VLEN * lo), (ko, st.out["ko"] + 8 * lo), (vo, st.out["vo"] + 8 * lo)):
            ctx.d2h(h, d)
        want = want_keys[lo:lo + n]
        v = v.reshape(n, VLEN)
        ok = (np.array_equal(k.reshape(n, 19), record_keys(want * 3)) and np.array_equal(v[:, :8].copy().view("<u8").reshape(-1).astype(np.int64), st.visible[want])
              and (v[:, 8:] == tail[None, :]).all() and np.array_equal(ko, (lo + np.arange(n + 1)) * 19) and np.array_equal(vo, (lo + np.arange(n + 1)) * VLEN))
        if not ok:
            return False
    return True


def read(st, packed, desc, limit, reps, label, want_keys, check=True):
    """want_keys: the key ordinals of the pairs the read must return, in order (from the numpy restatement)"""
    ctx, ms = st.ctx, st.ms
    want_pairs = want_keys.size
    rb, ro, rf = packed
    res = abi.MvccResult()
    R = len(ro) // 2

    def scan():
        _lib.check(ctx.lib.tsq_mvcc_scan(ms.h, rb.ctypes.data if rb.size else None, ro.ctypes.data, rf.ctypes.data, R, READ_TS, 1 if desc else 0, limit, C.byref(res), None), ms.h)

    def fetch():
        _lib.check(ctx.lib.tsq_mvcc_fetch(ms.h, st.out["k"], 19 * st.cap, st.out["ko"], st.out["v"], VLEN * st.cap, st.out["vo"]), ms.h)

    def both():
        scan()
        fetch()
    a, b, c = timed(scan, reps), timed(fetch, reps), timed(both, reps)
    assert res.n_pairs == want_pairs, (label, res.n_pairs, want_pairs)
    same = verify_rows(st, res.n_pairs, want_keys) if check else None
    assert same is not False, label
    moved = 9 * res.positions * st.n / st.K + 2 * (res.key_bytes + res.value_bytes)
    say("%-34s pairs %10d | scan %s | fetch %s | both %s | %7.3f GB %5.1f %% of 8 TB/s | rows %s" %
        (label, res.n_pairs, mmm(a), mmm(b), mmm(c), moved / 1e9, 100 * moved / (np.median(c) * HBM_BYTES_PER_MS), "identical" if same else "count only"))
    return float(np.median(c)), res


def gather_floor(st, reps):
    """(a): tsq_rows_gather of the visible rows' values, and of their keys"""
    ctx = st.ctx
    rows = ctx.alloc(st.rows.size * 8 + 64)
    ctx.h2d(rows, st.rows)
    gv, gvo = ctx.alloc(VLEN * st.rows.size + 64), ctx.alloc((st.rows.size + 1) * 8 + 64)
    gk, gko = ctx.alloc(19 * st.rows.size + 64), ctx.alloc((st.rows.size + 1) * 8 + 64)
    need = C.c_int64(0)

    def values():
        _lib.check(ctx.lib.tsq_rows_gather(ctx.h, st.dev["values"], st.value_bytes, st.dev["value_offsets"], st.n, rows, st.rows.size, gv, VLEN * st.rows.size, gvo,
                                           C.byref(need)), ctx.h)

    def keys():
        _lib.check(ctx.lib.tsq_rows_gather(ctx.h, st.dev["keys"], st.key_bytes, st.dev["key_offsets"], st.n, rows, st.rows.size, gk, 19 * st.rows.size, gko,
                                           C.byref(need)), ctx.h)
    a, b = timed(values, reps), timed(keys, reps)
    say("(a) tsq_rows_gather alone, %d rows: values %s | keys %s | sum of medians %.3f ms" % (st.rows.size, mmm(a), mmm(b), np.median(a) + np.median(b)))
    return float(np.median(a) + np.median(b)), (gv, gvo, gk, gko, rows)


def same_bytes(ctx, p, q, nbytes):
    step = 1 << 28
    for lo in range(0, nbytes, step):
        n = min(step, nbytes - lo)
        x, y = np.empty(n, dtype=np.uint8), np.empty(n, dtype=np.uint8)
        ctx.d2h(x, p + lo)
        ctx.d2h(y, q + lo)
        if not np.array_equal(x, y):
            return False
    return True


def run_store(ctx, kind, a, rng):
    t0 = time.perf_counter()
    st = Store(ctx, kind, int(a.keys), int(a.hot))
    say("== store %s: %d keys, %d versions (%.2f per key), %.2f GB of keys + values; built and uploaded in %.1f s, tsq_mvcc_create %.1f ms; visible at the read's ts: %d rows" %
        (kind, st.K, st.n, st.n / st.K, (st.key_bytes + st.value_bytes) / 1e9, time.perf_counter() - t0, st.create_ms, st.rows.size))
    try:
        whole = M.pack_ranges([(b"", b"")])
        floor, (gv, gvo, gk, gko, rows) = gather_floor(st, a.reps)
        vis_keys = np.flatnonzero(st.visible >= 0)
        t_asc, res = read(st, whole, False, -1, a.reps, "full range, ascending", vis_keys)
        nr = st.rows.size
        ok = (same_bytes(ctx, st.out["v"], gv, VLEN * nr) and same_bytes(ctx, st.out["vo"], gvo, 8 * (nr + 1)) and same_bytes(ctx, st.out["k"], gk, 19 * nr) and
              same_bytes(ctx, st.out["ko"], gko, 8 * (nr + 1)))
        say("    keys, values and both offset arrays of the ascending read == yardstick (a)'s output, byte for byte: %s; scan + fetch / (a) = %.2f" %
            ("yes" if ok else "NO", t_asc / floor))
        assert ok
        for p in (gv, gvo, gk, gko, rows):
            ctx.free(p)
        read(st, whole, True, -1, a.reps, "full range, descending", vis_keys[::-1])
        read(st, whole, False, 1, a.reps, "full range, limit 1", vis_keys[:1])
        # 2^10 ranges that tile the key space
        cuts = np.linspace(0, st.K, 1025).astype(np.int64)
        kb = record_keys(cuts * 3)
        read(st, M.pack_ranges([(bytes(kb[i]), bytes(kb[i + 1])) for i in range(1024)]), False, -1, a.reps, "2^10 ranges", vis_keys)
        # 2^20 point reads: every second one a key that is not there
        pk = rng.integers(0, st.K, 1 << 20)
        hs = pk * 3 + (np.arange(pk.size) & 1)
        keys = record_keys(hs)
        offs = np.empty(2 * pk.size + 1, dtype=np.int64)
        offs[0::2] = np.arange(pk.size + 1) * 19
        offs[1::2] = offs[2::2]
        packed = (keys.reshape(-1), offs, np.full(pk.size, abi.MVCC_POINT, dtype=np.uint32))
        want = pk[0::2][st.visible[pk[0::2]] >= 0]  # the hits, in the order asked (a key asked twice is returned twice)
        read(st, packed, False, -1, a.reps, "2^20 point reads, half miss", want)
        read(st, packed, False, 1, a.reps, "2^20 point reads, limit 1", want[:1])
        if kind in a.chains.split(","):
            say("-- A/B of TSQ_KNOB_MVCC_WAVE_CHAIN on this store (full range, ascending; 0 = never by the wave)")
            for knob in (0, 4, 16, 64, 256, 4096, 1 << 30):
                ctx.set_knob(abi.KNOB_MVCC_WAVE_CHAIN, knob)
                read(st, whole, False, -1, a.reps, "  chain threshold %d" % knob, vis_keys)
            ctx.set_knob(abi.KNOB_MVCC_WAVE_CHAIN)
    finally:
        st.free()
    say()


def host_yardstick(a):
    n = int(a.host_keys)
    say("== (c) the numpy restatement on one host core, %d keys" % n)
    for kind in a.stores.split(","):
        key, cts, types, m = entries_of(kind, 0, n, n // 2, int(a.hot))
        t0 = time.perf_counter()
        v = visible(cts, types, m, READ_TS)
        rows = v[v >= 0]
        ms = (time.perf_counter() - t0) * 1e3
        say("%-5s %d versions -> %d rows: verdicts %.1f ms (the copy of the rows' keys and values not included)" % (kind, cts.size, rows.size, ms))
    say()


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--keys", type=float, default=1e8)
    ap.add_argument("--hot", type=float, default=1e6)
    ap.add_argument("--host-keys", type=float, default=1e7)
    ap.add_argument("--stores", default="v1,v1.2,v3,hot")
    ap.add_argument("--chains", default="v3,hot")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--out", default="")
    ap.add_argument("--append", action="store_true", help="add to --out instead of replacing it (the stores of one profile measured in several runs)")
    ap.add_argument("--no-host", action="store_true", help="leave yardstick (c) out")
    a = ap.parse_args()
    rng = np.random.default_rng(21)
    say("tools/bench_mvcc_scan.py --keys %g --hot %g --host-keys %g --stores %s --chains %s --reps %d" % (a.keys, a.hot, a.host_keys, a.stores, a.chains, a.reps))
    say("ms per call, median [min .. max]; the GB column: 9 bytes per version of the keys examined + 2 x (key + value bytes returned)")
    say()
    with _lib.Context(0) as ctx:
        for kind in a.stores.split(","):
            run_store(ctx, kind, a, rng)
    if not a.no_host:
        host_yardstick(a)
    if a.out:
        os.makedirs(os.path.dirname(os.path.abspath(a.out)), exist_ok=True)
        with open(a.out, "a" if a.append else "w") as f:
            f.write("\n".join(LINES) + "\n")


if __name__ == "__main__":
    main()
