#!/usr/bin/env python3
"""A/B of GROUP BY over SIX key columns (tsq_agg_create_keys: the tsq_groupid front + an aggregate GROUP BY id, csrc/tsq_groupid.hip)
against the four-key GROUP BY over rows with the SAME groups: key columns 5 and 6 are functions of the first four, so both runs
build identical groups.  The yardstick leg uses only calls older libraries have too (tsq_agg_create), so this file also runs on a
build of the commit before the front: the new legs are skipped when the library lacks tsq_agg_create_keys.

Workload: --rows rows (default 1e8) generated in HBM (tsq_gen_column): BIGINT k0..k3 uniform in [0, m), k4 = hash(k0), k5 = hash(k1),
v uniform in [0, 1000); SELECT SUM(v), COUNT(*), FIRST_ROW(k0..k3) GROUP BY the keys.
  g1e3   m = 10, 10, 10, 1      1 000 groups
  g1e6   m = 32                 1 048 576 groups
  g1e7   m = 56                 9 834 496 groups
  str    m = 32, GROUP BY k0..k3, k4 and a 16-byte string (two hashed words of k1, k2): five BIGINT columns + one var-len column
Every group of every leg is checked against numpy (bincount over the composite of k0..k3).
Per case: ms of push + finish for both legs (device events, median [min .. max] of --reps passes after one warm-up), the front alone
(tsq_groupid_assign over the key columns: its own GPU time, tsq_groupid_stats) and the front's algorithmic bytes per row — the claim
pass reads N x 8 B of keys and writes 8 B, the flag pass reads 8 B and writes 1 B, the count pass reads 1 B, the resolve pass reads 8 B
and writes 8 B of id (slot reads not counted: the table is L2 resident for few groups) — as a fraction of 8 TB/s over the front's time.
   python tools/bench_groupid.py [--rows 1e8] [--reps 3] [--cases g1e3,g1e6,g1e7,str] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402

HBM_BYTES_PER_MS = 8e12 / 1e3
CASES = {"g1e3": (10, 10, 10, 1), "g1e6": (32,) * 4, "g1e7": (56,) * 4, "str": (32,) * 4}
M64 = np.uint64(0xFFFFFFFFFFFFFFFF)


def spec(kind, col, m=0, b=0):
    s = abi.GenSpec()
    s.kind, s.table, s.col, s.seed, s.m, s.b = kind, 11, col, 77, m, b
    return s


def splitmix64(x):
    with np.errstate(over="ignore"):
        x = x + np.uint64(0x9E3779B97F4A7C15)
        z = x
        z = (z ^ (z >> np.uint64(30))) * np.uint64(0xBF58476D1CE4E5B9)
        z = (z ^ (z >> np.uint64(27))) * np.uint64(0x94D049BB133111EB)
        return z ^ (z >> np.uint64(31))


def dev_col(ptr, tp, n, offsets=None):
    c = abi.Col()
    c.data, c.length, c.elem_size, c.type, c.flags = ptr, n, (-1 if tp == abi.BYTES else 8), tp, abi.COL_DEVICE
    c.offsets = offsets
    return c


class Table:
    """k0..k5, v (+ the string column of the `str` case) in HBM; k0..k3 and v also on the host for the check"""

    def __init__(self, ctx, n, mods, with_str):
        self.ctx, self.n, self.mods = ctx, n, mods
        self.ptr = [ctx.alloc(n * 8 + 64) for _ in range(7)]
        for c, m in enumerate(mods):
            ctx.gen_column(spec(abi.GEN_RAND_MOD, c, m), n, self.ptr[c])
        ctx.gen_column(spec(abi.GEN_HASH_OF_COL, 4, b=1), n, self.ptr[4], src=self.ptr[0])
        ctx.gen_column(spec(abi.GEN_HASH_OF_COL, 5, b=2), n, self.ptr[5], src=self.ptr[1])
        ctx.gen_column(spec(abi.GEN_RAND_MOD, 6, 1000), n, self.ptr[6])
        self.host = []
        for c in (0, 1, 2, 3, 6):
            h = np.zeros(n, np.int64)
            ctx.d2h(h, self.ptr[c])
            self.host.append(h)
        self.code = np.zeros(n, np.int64)  # the composite of k0..k3: the group of a row
        mul = 1
        for c, m in enumerate(mods):
            self.code += self.host[c] * mul
            mul *= m
        self.n_codes = mul
        self.sptr = self.soffs = None
        if with_str:  # 16-byte cells: splitmix64(k1 ^ 3), splitmix64(k2 ^ 4) — a function of the first four keys
            words = np.empty(2 * n, np.uint64)
            words[0::2] = splitmix64(self.host[1].view(np.uint64) ^ np.uint64(3))
            words[1::2] = splitmix64(self.host[2].view(np.uint64) ^ np.uint64(4))
            self.sptr, self.soffs = ctx.alloc(16 * n + 64), ctx.alloc(8 * (n + 1) + 64)
            ctx.h2d(self.sptr, words)
            ctx.h2d(self.soffs, np.arange(n + 1, dtype=np.int64) * 16)

    def cols(self, which):
        """tsq_col array of the input columns `which` (0..6 = k0..k5, v; 7 = the string)"""
        arr = (abi.Col * len(which))()
        for i, c in enumerate(which):
            arr[i] = dev_col(self.sptr, abi.BYTES, self.n, self.soffs) if c == 7 else dev_col(self.ptr[c], abi.I64, self.n)
        return arr

    def free(self):
        for p in self.ptr + [self.sptr, self.soffs]:
            self.ctx.free(p)


def agg_cfg(types, n_keys_in_cfg, est):
    """input: the key columns, then v; SUM(v), COUNT(*), FIRST_ROW(k0..k3)"""
    cfg = abi.AggCfg()
    v = len(types) - 1
    funcs = [(abi.AGG_SUM, v), (abi.AGG_COUNT, -1)] + [(abi.AGG_FIRSTROW, k) for k in range(4)]
    cfg.n_aggs = len(funcs)
    for i, (f, c) in enumerate(funcs):
        cfg.aggs[i].func, cfg.aggs[i].mode, cfg.aggs[i].arg_col, cfg.aggs[i].arg_col2, cfg.aggs[i].arg_type = f, abi.MODE_COMPLETE, c, -1, abi.I64
    cfg.n_input_cols = len(types)
    for i, t in enumerate(types):
        cfg.input_types[i] = t
    cfg.n_group_keys = n_keys_in_cfg
    for k in range(n_keys_in_cfg):
        cfg.group_key_col[k], cfg.group_key_type[k] = k, types[k]
    cfg.est_groups, cfg.max_chunk_size = est, 1024
    return cfg


def run_agg(ctx, tab, which, n_keys, reps, check):
    """push + finish of one device chunk; returns ([ms], stats of the last pass)"""
    lib, n = ctx.lib, tab.n
    types = [abi.BYTES if c == 7 else abi.I64 for c in which]
    cols = tab.cols(which)
    ms, st = [], abi.Stats()
    for it in range(reps + 1):
        h = C.c_void_p()
        if n_keys <= abi.MAX_GROUP_KEYS:
            cfg = agg_cfg(types, n_keys, tab.n_codes)
            _lib.check(lib.tsq_agg_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
        else:
            cfg = agg_cfg(types, 0, tab.n_codes)
            kc, kt = (C.c_int32 * n_keys)(*range(n_keys)), (C.c_int32 * n_keys)(*types[:n_keys])
            _lib.check(lib.tsq_agg_create_keys(ctx.h, C.byref(cfg), kc, kt, n_keys, C.byref(h)), ctx.h)
        try:
            ctx.sync()
            ctx.timer_start()
            _lib.check(lib.tsq_agg_push(h, cols, len(which), n), h)
            _lib.check(lib.tsq_agg_finish(h), h)
            t = ctx.timer_stop_ms()
            if it:
                ms.append(t)
            if it == reps:
                _lib.check(lib.tsq_agg_stats(h, C.byref(st)), h)
                check(pull_all(ctx, h))
        finally:
            lib.tsq_agg_destroy(h)
    return ms, st


def pull_all(ctx, h):
    """the six result columns on the host"""
    lib = ctx.lib
    g = C.c_int64(0)
    _lib.check(lib.tsq_agg_num_groups(h, C.byref(g)), h)
    cap = (g.value + 8) & ~7
    ptrs = [(ctx.alloc(cap * 8 + 64), ctx.alloc(cap // 8 + 64)) for _ in range(6)]
    try:
        oc = (abi.Col * 6)()
        for i, (d, bm) in enumerate(ptrs):
            oc[i] = dev_col(d, abi.I64, cap)
            oc[i].null_bitmap = bm
        n, eos = C.c_int64(0), C.c_int32(0)
        _lib.check(lib.tsq_agg_pull(h, oc, 6, cap, C.byref(n), C.byref(eos)), h)
        out = []
        for d, _ in ptrs:
            a = np.zeros(max(n.value, 1), np.int64)
            ctx.d2h(a, d)
            out.append(a[:n.value])
        return out
    finally:
        for d, bm in ptrs:
            ctx.free(d)
            ctx.free(bm)


def checker(tab):
    cnt = np.bincount(tab.code, minlength=tab.n_codes)
    sm = np.bincount(tab.code, weights=tab.host[4].astype(np.float64), minlength=tab.n_codes)  # (sums < 2^53: exact)
    n_groups = int((cnt > 0).sum())

    def check(res):
        s, c, k = res[0], res[1], res[2:6]
        code, mul = np.zeros(len(s), np.int64), 1
        for i, m in enumerate(tab.mods):
            code += k[i] * mul
            mul *= m
        assert len(s) == n_groups and len(np.unique(code)) == n_groups, "groups: %d, expected %d" % (len(s), n_groups)
        assert np.array_equal(c, cnt[code]) and np.array_equal(s, sm[code].astype(np.int64)), "a group's COUNT(*) / SUM(v) differs from numpy"
    return check, n_groups


def front_alone(ctx, tab, which_keys, reps):
    """tsq_groupid_assign over the key columns: GPU ms of the call (the handle's own events), collision rows, growths"""
    lib, n = ctx.lib, tab.n
    types = [abi.BYTES if c == 7 else abi.I64 for c in which_keys]
    cols = tab.cols(which_keys)
    ids = ctx.alloc(8 * n + 64)
    out = []
    try:
        for it in range(reps + 1):
            h = C.c_void_p()
            _lib.check(lib.tsq_groupid_create(ctx.h, (C.c_int32 * len(types))(*types), len(types), tab.n_codes, C.byref(h)), ctx.h)
            try:
                _lib.check(lib.tsq_groupid_assign(h, cols, len(types), n, C.c_void_p(ids)), h)
                rows, coll, reh, ms, g = C.c_int64(0), C.c_int64(0), C.c_int32(0), C.c_double(0), C.c_int64(0)
                _lib.check(lib.tsq_groupid_stats(h, C.byref(rows), C.byref(coll), C.byref(reh), C.byref(ms)), h)
                _lib.check(lib.tsq_groupid_count(h, C.byref(g)), h)
                if it:
                    out.append((ms.value, coll.value, reh.value, g.value))
            finally:
                lib.tsq_groupid_destroy(h)
    finally:
        ctx.free(ids)
    return out


def _mmm(v):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1e8")
    ap.add_argument("--reps", type=int, default=3)
    ap.add_argument("--cases", default=",".join(CASES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(float(a.rows))
    lines = ["%d device-resident rows; SUM(v), COUNT(*), FIRST_ROW(k0..k3); ms of push + finish: median [min .. max] of %d passes after one warm-up, device events" % (n, a.reps)]
    results = []
    with _lib.Context(0) as ctx:
        new = hasattr(ctx.lib, "tsq_agg_create_keys")
        for name in a.cases.split(","):
            tab = Table(ctx, n, CASES[name], name == "str")
            try:
                check, n_groups = checker(tab)
                keys6 = [0, 1, 2, 3, 4, 7] if name == "str" else [0, 1, 2, 3, 4, 5]
                r = {"case": name, "rows": n, "groups": n_groups}
                ms4, st4 = run_agg(ctx, tab, [0, 1, 2, 3, 6], 4, a.reps, check)
                r["four_keys_ms"] = ms4
                lines.append("%-5s %9d groups  four keys (yardstick) %s   route %d" % (name, n_groups, _mmm(ms4), st4.build_partitioned))
                if new:
                    ms6, st6 = run_agg(ctx, tab, keys6 + [6], 6, a.reps, check)
                    fr = front_alone(ctx, tab, keys6, a.reps)
                    fms = float(np.median([x[0] for x in fr]))
                    key_bytes = sum(16 + 8 if c == 7 else 8 for c in keys6)  # a string cell: its 16 bytes + an offset
                    per_row = (key_bytes + 8) + (8 + 1) + 1 + (8 + 8)
                    r.update({"six_keys_ms": ms6, "front_ms": [x[0] for x in fr], "front_collision_rows": fr[-1][1], "front_growths": fr[-1][2],
                              "front_bytes_per_row": per_row})
                    assert st6.build_partitioned == 5 and fr[-1][3] == n_groups
                    lines.append("%-5s %9d groups  six keys              %s   route %d; x %.2f of the yardstick" % (name, n_groups, _mmm(ms6), st6.build_partitioned,
                                                                                                                  float(np.median(ms6)) / float(np.median(ms4))))
                    lines.append("%-5s                   front alone (k_gid_claim, k_gid_flag, k_compact_count, k_compact_scan, k_gid_bind, k_gid_resolve + dictionary appends) "
                                 "%8.3f ms; %d B/row algorithmic = %.3f of 8 TB/s; collision rows %d, growths %d" %
                                 (name, fms, per_row, per_row * n / (fms * HBM_BYTES_PER_MS), fr[-1][1], fr[-1][2]))
                results.append(r)
                print("\n".join(lines[-3:] if new else lines[-1:]), flush=True)
            finally:
                tab.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
            f.write(json.dumps(results) + "\n")
    print(json.dumps({"bench": "groupid", "new_legs": new, "cases": len(results)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
