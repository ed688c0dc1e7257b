#!/usr/bin/env python3
"""The duplicate-key checker (tsq_dupcheck_* + tsq_rows_equal, csrc/tsq_dupcheck.hip) on device columns: REPLACE .. SELECT's row logic and
INSERT .. SELECT's check, against a store of --store rows (default 1e8), in the same run as the two routes that exist without it.

Store: handles 0 .. S - 1 (ascending); the BIGINT unique index over v = handle, the string unique index over the 8 big-endian bytes of the
handle (so both key orders are the handle order); keys by tsq_indexkeys_encode.  The store is given to tsq_dupcheck_create ONCE per
configuration (its time is reported on its own line: the copy, the order checks, the search index) and every statement then starts with
tsq_dupcheck_reset.
Statement: n rows (2^14, 2^20, 2^22); a fraction p (0, 1 %, 50 %) of them carries the handle AND the unique value of a stored row (another
row's value for every second one, so that half of the colliding rows are changed and remove two stored rows, half of them are the stored
row cell for cell), the rest is new; no two rows of a statement share a key (in-batch groups are all singletons: the grouping and sort
passes run at full cost, their results are trivial).
Per statement, ms of WHOLE CALLS from device events (tsq_timer_*), median [min .. max] of --reps statements after one warm-up:
  push, match, the two tsq_rows_equal calls, resolve, and their sum; for INSERT mode push + match.
Phases inside match are measured STAND-ALONE on the same keys in the same run (not as internal timers): tsq_groupid_assign per stream
(grouping; with a tsq_groupid_count read-back the checker does not pay), a tsq_sort of the n raw handles per stream (sort; the checker
sorts id << 32 | row words: same width and count, other bit patterns); search + verdict = match minus those approximations.
Beside it: (a) what the operators that existed before answer — tsq_lookup_task over the statement's handles (does any exist?) and
tsq_groupid_assign / tsq_groupid_count per stream (fewer groups than rows?): a yes / no, no row, no stream, no REPLACE;
(b) one host core: numpy searchsorted + unique over the same keys (PK and BIGINT index only), on --host-rows rows.
Bytes that must move per statement row: every stream's key once (8 B or the encoded key), the three candidate words, the flags and the
handle out (35 B); the fraction is of 8 TB/s.
   python tools/bench_dupcheck.py [--store 1e8] [--reps 5] [--host-rows 1048576] [--out FILE]"""
import argparse
import ctypes as C
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import dupcheck as D  # noqa: E402
from tinysql_amd import tablecodec  # noqa: E402
from tinysql_amd.gpu_pipeline import DeviceChunk, DeviceColumn  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3
TABLE_ID = 41


def _mmm(v):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(v)), min(v), max(v))


def timed(ctx, fn):
    ctx.sync()
    ctx.timer_start()
    fn()
    return ctx.timer_stop_ms()


def int_col(ctx, host):
    c = DeviceColumn(ctx, abi.I64, len(host), with_bitmap=False)
    ctx.h2d(c.data, np.ascontiguousarray(host, dtype=np.int64))
    return c


def str8_col(ctx, host):
    """the 8 big-endian bytes of every value as a string cell"""
    n = len(host)
    c = DeviceColumn(ctx, abi.BYTES, n, with_bitmap=False, cap_bytes=8 * n)
    ctx.h2d(c.data, np.ascontiguousarray(host.astype(">i8")).view(np.uint8))
    ctx.h2d(c.offsets, np.arange(n + 1, dtype=np.int64) * 8)
    return c


def statement(n, S, p, seed):
    """-> (handles, unique values): a fraction p of the rows meets stored rows"""
    rng = np.random.default_rng(seed)
    hit = rng.random(n) < p
    stride = 7919  # (coprime to the store sizes used: distinct stored rows for distinct statement rows)
    stored = (np.arange(n, dtype=np.int64) * stride) % S
    fresh = S + np.arange(n, dtype=np.int64)
    h = np.where(hit, stored, fresh)
    other = (stored + S // 2) % S  # another stored row's value for every second colliding row
    v = np.where(hit & (np.arange(n) % 2 == 1), other, h)
    return h, v


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--store", default="1e8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--host-rows", default="1048576")
    ap.add_argument("--sizes", default="16384,1048576,4194304")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    S, hn = int(float(a.store)), int(float(a.host_rows))
    sizes = [int(x) for x in a.sizes.split(",")]
    lines = []

    def say(line):
        lines.append(line)
        print(line, flush=True)

    with _lib.Context(0) as ctx:
        lib = ctx.lib
        say("store: %d rows; statements of %s rows; ms of whole calls from device events, median [min .. max] of %d statements after one warm-up"
            % (S, ", ".join(map(str, sizes)), a.reps))
        sh = np.arange(S, dtype=np.int64)
        d_sh = int_col(ctx, sh)
        s_int = tablecodec.GenIndexKeys(ctx, TABLE_ID, 1, True, DeviceChunk([d_sh], S), d_sh.data)
        d_ss = str8_col(ctx, sh)
        s_str = tablecodec.GenIndexKeys(ctx, TABLE_ID, 2, True, DeviceChunk([d_ss], S), d_sh.data)
        d_ss.free()
        configs = [("PK handle only", []), ("PK + BIGINT unique index", [("int", s_int)]), ("PK + 8-byte string unique index", [("str", s_str)])]
        table = C.c_void_p()
        _lib.check(lib.tsq_lookup_create(ctx.h, C.c_void_p(d_sh.data), S, abi.COL_DEVICE, C.byref(table)), ctx.h)
        for name, idx in configs:
            streams = [D.HandleStream(d_sh.data, S)] + [D.IndexStream(kv.keys, kv.key_offsets, kv.nbytes, d_sh.data, S) for _, kv in idx]
            t0 = time.perf_counter()
            chk = {m: D.DupChecker(ctx, streams, m) for m in (abi.DUP_REPLACE, abi.DUP_INSERT)}
            ctx.sync()
            say("")
            say("== %s: tsq_dupcheck_create %.1f ms per handle (host clock, once per store: copy, order checks, search index); store key bytes/row %s"
                % (name, (time.perf_counter() - t0) * 500, [kv.nbytes // S for _, kv in idx]))
            for n in sizes:
                for p in (0.0, 0.01, 0.5):
                    h, v = statement(n, S, p, n)
                    d_h, d_v = int_col(ctx, h), int_col(ctx, v)
                    cols = [d_h, d_v]
                    kvs, kcols = [], []
                    for kind, _ in idx:
                        kc = d_v if kind == "int" else str8_col(ctx, v)
                        kcols.append(kc)
                        kvs.append(tablecodec.GenIndexKeys(ctx, TABLE_ID, 1 if kind == "int" else 2, True, DeviceChunk([kc], n), d_h.data))
                    keys = [d_h.data] + [(kv.keys, kv.key_offsets, kv.nbytes, kv.distinct) for kv in kvs]
                    key_bytes = 8 * n + sum(kv.nbytes for kv in kvs)
                    outs = [D.DevArray(ctx, nbytes=8 * n) for _ in range(6)] + [D.DevArray(ctx, nbytes=n) for _ in range(4)]
                    c_row, c_h, c_o, hs_out, r_h, r_o, f1, f2, added, put = outs
                    # the stored rows (handle, v = handle) as a chunk: EqualDatums reads them through the candidates' ordinals
                    old = [d_sh.col(S), d_sh.col(S)]
                    new = [c.col(n) for c in cols]
                    ph = {k: [] for k in ("push", "match", "equal", "resolve", "insert push+match", "group", "sort")}
                    res = None
                    for it in range(a.reps + 1):
                        r = chk[abi.DUP_REPLACE]
                        r.reset()
                        t = [timed(ctx, lambda: r.push(keys, n)), timed(ctx, lambda: r.match_replace(c_row.p, c_h.p, c_o.p))]

                        def equal():
                            D.rows_equal(ctx, new, None, new, c_row.p, n, f1.p)
                            D.rows_equal(ctx, new, None, old, c_o.p, n, f2.p)
                        t.append(timed(ctx, equal))
                        # (statement-row candidates are rare chance meetings here and count as changed: the stored-row flags are the equality flags)
                        t.append(timed(ctx, lambda: r.resolve(f2.p, 0, added.p, put.p, hs_out.p, r_h.p, r_o.p, n)))
                        res = r.resolve(f2.p, 0, added.p, put.p, hs_out.p, r_h.p, r_o.p, n)
                        i = chk[abi.DUP_INSERT]
                        i.reset()

                        def ins():
                            i.push(keys, n)
                            return i.match_insert()
                        t.append(timed(ctx, ins))
                        # stand-alone: grouping and sort of the same keys
                        gids = D.DevArray(ctx, nbytes=8 * n)

                        def group():
                            for k, key in enumerate(keys):
                                g = C.c_void_p()
                                tp = (C.c_int32 * 1)(abi.I64 if k == 0 else abi.BYTES)
                                _lib.check(lib.tsq_groupid_create(ctx.h, tp, 1, n, C.byref(g)), ctx.h)
                                col = (abi.Col * 1)(d_h.col(n) if k == 0 else DeviceColumn(ctx, abi.BYTES, n, data=key[0], offsets=key[1], cap_bytes=key[2]).col(n))
                                _lib.check(lib.tsq_groupid_assign(g, col, 1, n, C.c_void_p(gids.p)), g)
                                ng = C.c_int64(0)
                                _lib.check(lib.tsq_groupid_count(g, C.byref(ng)), g)
                                lib.tsq_groupid_destroy(g)
                        t.append(timed(ctx, group))

                        def sort():
                            for _ in keys:
                                cfg = abi.SortCfg()
                                cfg.n_cols, cfg.n_keys, cfg.limit_count, cfg.max_chunk_size = 1, 1, -1, 1024
                                cfg.col_types[0] = abi.I64
                                sh_ = C.c_void_p()
                                _lib.check(lib.tsq_sort_create(ctx.h, C.byref(cfg), C.byref(sh_)), ctx.h)
                                col = (abi.Col * 1)(d_h.col(n))
                                _lib.check(lib.tsq_sort_push(sh_, col, 1, n), sh_)
                                _lib.check(lib.tsq_sort_finish(sh_), sh_)
                                out = (abi.Col * 1)(DeviceColumn(ctx, abi.I64, n, data=gids.p, bitmap=c_row.p).col(n))
                                got, eos = C.c_int64(0), C.c_int32(0)
                                _lib.check(lib.tsq_sort_pull(sh_, out, 1, n, C.byref(got), C.byref(eos)), sh_)
                                lib.tsq_sort_destroy(sh_)
                        t.append(timed(ctx, sort))
                        gids.free()
                        if it:
                            for k, x in zip(ph, t):
                                ph[k].append(x)
                    whole = [sum(x) for x in zip(ph["push"], ph["match"], ph["equal"], ph["resolve"])]
                    moved = key_bytes + 35 * n
                    med = float(np.median(whole))
                    say("n = %8d  collide %4.1f %%  REPLACE %s ms = %7.1f Mrows/s, %.4f of 8 TB/s on %d B/row  (added %d, stored rows removed %d, affected %d)"
                        % (n, 100 * p, _mmm(whole), n / med / 1e3, moved / (med * HBM_BYTES_PER_MS), moved // n, res.n_added, res.n_removed_store, res.affected))
                    say("      push %s   match %s   rows_equal x2 %s   resolve %s" % tuple(_mmm(ph[k]) for k in ("push", "match", "equal", "resolve")))
                    say("      inside match, stand-alone: grouping %s   sort %s   search + verdict (the rest) %8.3f"
                        % (_mmm(ph["group"]), _mmm(ph["sort"]), float(np.median(ph["match"])) - float(np.median(ph["group"])) - float(np.median(ph["sort"]))))
                    say("      INSERT mode push + match %s ms" % _mmm(ph["insert push+match"]))
                    # (a) the operators that existed before: lookup (any stored handle?) + group count per stream (a yes / no)
                    ra = []
                    for it in range(a.reps + 1):
                        def route_a():
                            nf = C.c_int64(0)
                            _lib.check(lib.tsq_lookup_task(table, C.c_void_p(d_h.data), n, abi.COL_DEVICE, 0, C.c_void_p(c_row.p), C.c_void_p(c_h.p), C.byref(nf)), table)
                            gids = D.DevArray(ctx, nbytes=8 * n)
                            for k, key in enumerate(keys):
                                g = C.c_void_p()
                                tp = (C.c_int32 * 1)(abi.I64 if k == 0 else abi.BYTES)
                                _lib.check(lib.tsq_groupid_create(ctx.h, tp, 1, n, C.byref(g)), ctx.h)
                                col = (abi.Col * 1)(d_h.col(n) if k == 0 else DeviceColumn(ctx, abi.BYTES, n, data=key[0], offsets=key[1], cap_bytes=key[2]).col(n))
                                _lib.check(lib.tsq_groupid_assign(g, col, 1, n, C.c_void_p(gids.p)), g)
                                ng = C.c_int64(0)
                                _lib.check(lib.tsq_groupid_count(g, C.byref(ng)), g)
                                lib.tsq_groupid_destroy(g)
                            gids.free()
                        x = timed(ctx, route_a)
                        if it:
                            ra.append(x)
                    say("      (a) tsq_lookup_task on the handles + group count per stream (yes / no only; the index streams' store is not searched): %s ms" % _mmm(ra))
                    for o in outs:
                        o.free()
                    for kv in kvs:
                        kv.free()
                    for kc in kcols:
                        if kc is not d_v:
                            kc.free()
                    d_h.free()
                    d_v.free()
            for c in chk.values():
                c.close()
        # (b) one host core
        say("")
        h, v = statement(hn, S, 0.01, 1)
        t0 = time.perf_counter()
        pos = np.searchsorted(sh, h)
        hit_h = sh[np.minimum(pos, S - 1)] == h
        pos = np.searchsorted(sh, v)
        hit_v = sh[np.minimum(pos, S - 1)] == v
        dup = len(np.unique(h)) < hn or len(np.unique(v)) < hn
        ms = (time.perf_counter() - t0) * 1e3
        say("(b) one host core, numpy (searchsorted of handle and BIGINT value in the store + unique of both; yes / no + the hit masks), %d rows, 1 %% colliding: "
            "%.1f ms = %.1f Mrows/s  (hits %d / %d, in-batch duplicate %s)" % (hn, ms, hn / ms / 1e3, int(hit_h.sum()), int(hit_v.sum()), dup))
        lib.tsq_lookup_destroy(table)
        s_int.free()
        s_str.free()
        d_sh.free()
    if a.out:
        with open(a.out, "w") as f:
            f.write("\n".join(lines) + "\n")


if __name__ == "__main__":
    main()
