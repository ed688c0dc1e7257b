#!/usr/bin/env python3
"""A/B of a join on (bigint, varstring) keys WITH an OtherCondition: the direct route (TSQ_KNOB_KEYREC_CONDS = 0, what every such join
took before the key-record route learnt conditions) against the key-record route with the condition inside its probe kernel
(csrc/tsq_keyrec.h k_kr_probe<VERIFY, true>, TSQ_KNOB_KEYREC_CONDS = 1), alternating in one process; tsq_stats.probe_route proves
which route ran.

Workload: the key shape of tools/bench_sides.py extra_string_key_join — build rows k = a permutation of 0 .. n-1, probe rows k uniform in
[0, 2n) (hit ratio 0.5, one candidate per hit), s a 16-byte binary string derived from k — plus a BIGINT payload v uniform in [0, 2^20)
on both sides; the condition is probe.v < build.v (about half of the candidates pass).  Radix FORCED, so that every size takes the
route the knob allows.  Modes: inner COUNT(*), inner materialising, left outer materialising (six output columns, two of them strings).
Per mode one join handle per variant (build side pushed, one warm-up probe pass each); then --reps timed probe passes per variant,
ALTERNATING between the two handles (the timed passes' rows stay in the handle, un-pulled, until it is destroyed); device events
(tsq_timer_start / tsq_timer_stop_ms), median and min-max.  Before timing, the variants' outputs are compared: the row count and an order-independent fingerprint of the warm-up pass's rows (sum and xor over the rows
of a 64-bit mix of the fixed-width cells, their NULL flags and each string cell's length and byte sum).
--ref-shape adds the reference benchmark's shape: (bigint, 5 KiB varstring) keys, 1e5 x 1e5 rows (executor/benchmark_test.go:328-360).
   python tools/bench_keyrec_conds.py [--sizes 65536,262144,...] [--reps 7] [--ref-shape] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import expression as E  # noqa: E402

SIZES = [1 << 16, 1 << 18, 1 << 20, 1 << 22, 10_000_000]
VARIANTS = (("direct", 0, abi.ROUTE_DIRECT), ("keyrec_conds", 1, abi.ROUTE_KEYREC))
MODES = (("count_inner", abi.JOIN_INNER, True), ("rows_inner", abi.JOIN_INNER, False), ("rows_left_outer", abi.JOIN_LEFT_OUTER, False))
TYPES = [abi.I64, abi.BYTES, abi.I64]
M = [np.uint64(m) for m in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93, 0x27D4EB2F165667C5, 0x85EBCA77C2B2AE63)]


def _strings(k, width):
    """width bytes per cell (a multiple of 8): two 64-bit mixes of the bigint, then a filler that is the same in every cell"""
    a = (k.astype(np.uint64) * np.uint64(0x9E3779B97F4A7C15)) ^ np.uint64(0x1234567)
    b = (k.astype(np.uint64) + np.uint64(77)) * np.uint64(0xC2B2AE3D27D4EB4F)
    out = np.empty((len(k), width // 8), np.uint64)
    out[:, 2:] = np.arange(width // 8 - 2, dtype=np.uint64) * np.uint64(0x0101010101010101)
    out[:, 0], out[:, 1] = a, b
    return out.view(np.uint8).reshape(-1)


class Side:
    def __init__(self, ctx, k, v, width):
        self.ctx, self.n, self.dev = ctx, len(k), []
        offs = np.arange(self.n + 1, dtype=np.int64) * width
        c = (abi.Col * 3)()
        for i, arr in ((0, k.astype(np.int64)), (2, v.astype(np.int64))):
            c[i].data, c[i].length, c[i].elem_size, c[i].type, c[i].flags = self._up(arr), self.n, 8, abi.I64, abi.COL_DEVICE
        c[1].data, c[1].offsets, c[1].length, c[1].elem_size, c[1].type, c[1].flags = self._up(_strings(k, width)), self._up(offs), self.n, -1, abi.BYTES, abi.COL_DEVICE
        self.cols = c

    def _up(self, arr):
        p = self.ctx.alloc(arr.nbytes + 64)
        self.ctx.h2d(p, np.ascontiguousarray(arr))
        self.dev.append(p)
        return p

    def free(self):
        for p in self.dev:
            self.ctx.free(p)


def _fingerprint(ctx, h, pull_rows):
    """drains the join's rows (device-resident pulls, copied to the host pull by pull) and mixes them: (rows, sum, xor)"""
    lib = ctx.lib
    types = TYPES + TYPES
    got, s, x = 0, 0, 0
    while True:
        pn, pb = C.c_int64(0), (C.c_int64 * 6)()
        _lib.check(lib.tsq_join_peek(h, pull_rows, C.byref(pn), pb, 6), h)
        out = (abi.Col * 6)()
        dev = []
        try:
            for i, tp in enumerate(types):
                nbytes = pb[i] if tp == abi.BYTES else pull_rows * 8
                ptrs = [ctx.alloc(nbytes + 64), ctx.alloc(pull_rows // 8 + 64), ctx.alloc((pull_rows + 1) * 8 + 64) if tp == abi.BYTES else None]
                dev.append(ptrs)
                out[i].data, out[i].null_bitmap, out[i].offsets = ptrs
                out[i].length, out[i].elem_size, out[i].type, out[i].flags = pull_rows, -1 if tp == abi.BYTES else 8, tp, abi.COL_DEVICE
            nn, eos = C.c_int64(0), C.c_int32(0)
            _lib.check(lib.tsq_join_pull(h, out, 6, pull_rows, C.byref(nn), C.byref(eos)), h)
            n = nn.value
            if n == 0:
                return got, s, x
            ctx.sync()
            acc = np.zeros(n, np.uint64)
            for i, tp in enumerate(types):
                raw = np.empty((n + 7) // 8, np.uint8)
                ctx.d2h(raw, dev[i][1])
                notnull = np.unpackbits(raw, bitorder="little")[:n].astype(bool)
                if tp == abi.BYTES:
                    offs = np.empty(n + 1, np.int64)
                    ctx.d2h(offs, dev[i][2])
                    data = np.empty(max(int(offs[n]), 1), np.uint8)
                    ctx.d2h(data, dev[i][0])
                    csum = np.concatenate([np.zeros(1, np.uint64), np.cumsum(data[:offs[n]], dtype=np.uint64)])
                    cells = (csum[offs[1:]] - csum[offs[:-1]]) * np.uint64(1 << 20) + (offs[1:] - offs[:-1]).astype(np.uint64)
                else:
                    cells = np.empty(n, np.uint64)
                    ctx.d2h(cells, dev[i][0])
                cells = np.where(notnull, cells, np.uint64(0x5bd1e995 + i))  # (the bytes of a NULL cell are unspecified)
                acc += (cells ^ (cells >> np.uint64(31))) * M[i] + notnull.astype(np.uint64) * np.uint64(i + 1)
            acc ^= acc >> np.uint64(29)
            acc *= M[1]
            acc ^= acc >> np.uint64(32)
            s = (s + int(acc.sum(dtype=np.uint64))) & 0xFFFFFFFFFFFFFFFF
            x ^= int(np.bitwise_xor.reduce(acc))
            got += n
        finally:
            for ptrs in dev:
                for p in ptrs:
                    if p:
                        ctx.free(p)


def run_mode(ctx, build, probe, jt, count_only, reps, pull_rows):
    lib = ctx.lib
    keep = []
    cfg = abi.JoinCfg()
    cfg.join_type, cfg.build_is_right, cfg.n_keys, cfg.n_build_cols, cfg.n_probe_cols = jt, 1, 2, 3, 3
    for i, t in enumerate(TYPES):
        cfg.build_types[i] = cfg.probe_types[i] = t
    for i in range(2):
        cfg.build_key_idx[i] = cfg.probe_key_idx[i] = i
    conds = E.compile_list([E.ScalarFunction("lt", E.Column(2, abi.I64), E.Column(5, abi.I64))])  # probe.v < build.v over probe || build
    keep.append(conds)
    cfg.other_conds, cfg.n_other_conds = conds, 1
    handles, res = {}, {}
    try:
        for name, knob, route in VARIANTS:  # the build side, one warm-up pass, the output check
            with ctx.knobs(KEYREC_CONDS=knob):
                h = C.c_void_p()
                _lib.check(lib.tsq_join_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
                handles[name] = h
                _lib.check(lib.tsq_join_set_radix(h, abi.RADIX_FORCE), h)
                _lib.check(lib.tsq_join_build_push(h, build.cols, 3, build.n), h)
                _lib.check(lib.tsq_join_build_finish(h), h)
                if count_only:
                    _lib.check(lib.tsq_join_set_count_only(h, 1), h)
                _lib.check(lib.tsq_join_probe_push(h, probe.cols, 3, probe.n, None), h)
                st = abi.Stats()
                _lib.check(lib.tsq_join_stats(h, C.byref(st)), h)
                if count_only:
                    c = C.c_int64(0)
                    _lib.check(lib.tsq_join_count(h, C.byref(c)), h)
                    fp = (c.value, 0, 0)
                else:
                    fp = _fingerprint(ctx, h, pull_rows)
                res[name] = {"rows": fp[0], "fingerprint": "%d:%016x:%016x" % fp, "route": int(st.probe_route), "route_ok": int(st.probe_route) == route, "ms": []}
        res["identical"] = res["direct"]["fingerprint"] == res["keyrec_conds"]["fingerprint"] and all(res[n]["route_ok"] for n, _, _ in VARIANTS)
        for _ in range(reps):
            for name, knob, _ in VARIANTS:
                h = handles[name]
                with ctx.knobs(KEYREC_CONDS=knob):
                    ctx.sync()
                    ctx.timer_start()
                    _lib.check(lib.tsq_join_probe_push(h, probe.cols, 3, probe.n, None), h)
                    res[name]["ms"].append(ctx.timer_stop_ms())
        return res
    finally:
        for h in handles.values():
            lib.tsq_join_destroy(h)


def _mmm(v):
    return "%9.3f [%9.3f .. %9.3f]" % (float(np.median(v)), min(v), max(v))


def _verdict(a, b):
    """the rule of the A/B: b is `no slower` than a when its median lies within a's min-max spread (or below it)"""
    mb = float(np.median(b))
    return "faster" if mb < min(a) else ("same" if mb <= max(a) else "slower")


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--modes", default=",".join(m[0] for m in MODES))
    ap.add_argument("--ref-shape", action="store_true", help="also (bigint, 5 KiB varstring) keys, 1e5 x 1e5 rows")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    shapes = [(int(float(s)), 16) for s in a.sizes.split(",") if s] + ([(100_000, 5120)] if a.ref_shape else [])
    lines = ["(bigint, varstring) keys, build k = permutation, probe k uniform in [0, 2n), payload v; OtherCondition probe.v < build.v; radix FORCED",
             "ms per probe pass against the prepared build side: median [min .. max] of %d alternating repetitions, device events" % a.reps,
             "%-10s %-6s %-16s %-13s %5s %10s  %-36s %-8s %s" % ("rows/side", "strlen", "mode", "variant", "route", "rows", "probe pass ms", "vs direct", "fingerprint")]
    results = []
    with _lib.Context(0) as ctx:
        for n, width in shapes:
            rng = np.random.default_rng(3)
            build = Side(ctx, rng.permutation(n), rng.integers(0, 1 << 20, n), width)
            probe = Side(ctx, rng.integers(0, 2 * n, n), rng.integers(0, 1 << 20, n), width)
            try:
                for mode, jt, count_only in MODES:
                    if mode not in a.modes.split(","):
                        continue
                    r = run_mode(ctx, build, probe, jt, count_only, a.reps, (1 << 20) if width == 16 else (1 << 13))
                    r.update({"rows_per_side": n, "strlen": width, "mode": mode})
                    results.append(r)
                    for name, _, _ in VARIANTS:
                        v = r[name]
                        vs = "" if name == "direct" else _verdict(r["direct"]["ms"], v["ms"])
                        lines.append("%-10d %-6d %-16s %-13s %5d %10d  %-36s %-8s %s" % (n, width, mode, name, v["route"], v["rows"], _mmm(v["ms"]), vs, v["fingerprint"]))
                    lines.append("%-10d %-6d %-16s outputs identical and routes as asked: %s" % (n, width, mode, r["identical"]))
                    print("\n".join(lines[-3:]), flush=True)
            finally:
                build.free()
                probe.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
            f.write(json.dumps(results) + "\n")
    ok = all(r["identical"] for r in results)
    print(json.dumps({"bench": "keyrec_conds", "all_identical": ok, "cases": len(results)}))
    return 0 if ok else 1


if __name__ == "__main__":
    sys.exit(main())
