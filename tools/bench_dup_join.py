#!/usr/bin/env python3
"""A/B of the materialising packed join over a build side WITH duplicate keys: the sorted-build-columns variant (TSQ_KNOB_DA_LDS_DUP = 0)
against the build side in LDS (csrc/tsq_damat_dup.h, TSQ_KNOB_DA_LDS_DUP = 2), alternating in one process.

Workload: SURVEY.md 8(d) `J-dup`, device-generated (tsq_gen_column, seed 42): build keys r(i, 0) mod (N_b / 4) — multiplicity 4 —, probe
keys uniform over the same range with N_p = N_b / 4 rows, (k, v) on both sides, four output columns, about N_b output rows.  Radix and
key packing are FORCED so that every size takes the packed route (AUTO leaves batches under 4 Mi rows to the direct route).
Per size and variant, after one warm-up of each: --reps repetitions of (i) ONE PASS = build_push + build_finish + the first probe_push
(everything the route prepares on the build side is in there) and (ii) a REPEATED probe pass against the prepared build side; device
events (tsq_timer_start / tsq_timer_stop_ms), median and min-max.  Before timing, the two variants' outputs are compared: the row count
and an order-independent fingerprint (sum and xor over the rows of a 64-bit mix of each row's cells and NULL flags).
   python tools/bench_dup_join.py [--sizes 65536,262144,...] [--reps 7] [--outer-at 100000000] [--out FILE]"""
import argparse
import ctypes as C
import json
import os
import sys

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402

SIZES = [1 << 16, 1 << 18, 1 << 20, 1 << 22, 1 << 24, 100_000_000]
VARIANTS = (("sorted_columns", 0), ("lds_dup", 2))


def _spec(kind, **kw):
    s = abi.GenSpec()
    s.kind, s.seed = kind, 42
    for k, v in kw.items():
        setattr(s, k, v)
    return s


def _col(ptr, rows, bm=None):
    c = abi.Col()
    c.data, c.length, c.elem_size, c.type, c.flags = ptr, rows, 8, abi.I64, abi.COL_DEVICE
    if bm:
        c.null_bitmap = bm
    return c


def _fingerprint(ctx, h):
    """pulls every row of the join device-resident, 8 Mi rows a pull, and mixes each pull on the host: (rows, sum, xor)"""
    lib = ctx.lib
    step = 1 << 23
    bufs = [ctx.alloc(step * 8 + 64) for _ in range(4)]
    bms = [ctx.alloc(step // 8 + 64) for _ in range(4)]
    mul = [np.uint64(m) for m in (0x9E3779B97F4A7C15, 0xC2B2AE3D27D4EB4F, 0x165667B19E3779F9, 0xD6E8FEB86659FD93)]
    got, s, x = 0, 0, 0
    try:
        while True:
            out = (abi.Col * 4)()
            for i in range(4):
                out[i].data, out[i].null_bitmap = bufs[i], bms[i]
                out[i].length, out[i].elem_size, out[i].type, out[i].flags = step, 8, abi.I64, abi.COL_DEVICE
            nn, eos = C.c_int64(0), C.c_int32(0)
            _lib.check(lib.tsq_join_pull(h, out, 4, step, C.byref(nn), C.byref(eos)), h)
            n = nn.value
            if n == 0:
                break
            ctx.sync()
            acc = np.zeros(n, np.uint64)
            for i in range(4):
                cells = np.empty(n, np.uint64)
                ctx.d2h(cells, bufs[i])
                raw = np.empty((n + 7) // 8, np.uint8)
                ctx.d2h(raw, bms[i])
                nnull = np.unpackbits(raw, bitorder="little")[:n].astype(bool)
                cells = np.where(nnull, cells, np.uint64(0x5bd1e995 + i))  # (the bytes of a NULL cell are unspecified)
                acc += (cells ^ (cells >> np.uint64(31))) * mul[i] + nnull.astype(np.uint64) * np.uint64(i + 1)
            acc ^= acc >> np.uint64(29)
            acc *= mul[1]
            acc ^= acc >> np.uint64(32)
            s = (s + int(acc.sum(dtype=np.uint64))) & 0xFFFFFFFFFFFFFFFF
            x ^= int(np.bitwise_xor.reduce(acc))
            got += n
        return got, s, x
    finally:
        for p in bufs + bms:
            ctx.free(p)


def run_size(ctx, nb, reps, outer):
    lib = ctx.lib
    keys, npr = nb // 4, nb // 4
    bk, bv, pk, pv = ctx.alloc(nb * 8), ctx.alloc(nb * 8), ctx.alloc(npr * 8), ctx.alloc(npr * 8)
    bms = []
    try:
        ctx.gen_column(_spec(abi.GEN_RAND_MOD, table=2, col=0, m=keys), nb, bk)
        ctx.gen_column(_spec(abi.GEN_RAND_MOD, table=1, col=0, m=keys), npr, pk)
        if outer:  # 3 % NULL probe keys, 3 % NULL payload cells on both sides
            bms = [ctx.alloc(npr // 8 + 64), ctx.alloc(npr // 8 + 64), ctx.alloc(nb // 8 + 64)]
            tmp = ctx.alloc(npr * 8)
            ctx.gen_column(_spec(abi.GEN_RAND_MOD, table=4, col=11, m=7, null_pct=3), npr, tmp, null_bitmap=bms[0])
            ctx.sync()
            ctx.free(tmp)
        ctx.gen_column(_spec(abi.GEN_RAND_MOD, table=2, col=1, m=1 << 40, null_pct=3 if outer else 0), nb, bv, null_bitmap=bms[2] if outer else None)
        ctx.gen_column(_spec(abi.GEN_RAND_MOD, table=1, col=1, m=1 << 40, null_pct=3 if outer else 0), npr, pv, null_bitmap=bms[1] if outer else None)
        ctx.sync()
        bcols = (abi.Col * 2)(_col(bk, nb), _col(bv, nb, bms[2] if outer else None))
        pcols = (abi.Col * 2)(_col(pk, npr, bms[0] if outer else None), _col(pv, npr, bms[1] if outer else None))
        cfg = abi.JoinCfg()
        cfg.join_type, cfg.build_is_right, cfg.n_keys, cfg.n_build_cols, cfg.n_probe_cols = abi.JOIN_LEFT_OUTER if outer else abi.JOIN_INNER, 1, 1, 2, 2
        for i in range(2):
            cfg.build_types[i] = cfg.probe_types[i] = abi.I64

        def one(knob, passes, fingerprint=False):
            """one join: build + `passes` probe pushes; returns (ms of build + first pass, ms of the last pass, stats, rows[, fingerprint])"""
            h = C.c_void_p()
            with ctx.knobs(DA_LDS_DUP=knob):
                _lib.check(lib.tsq_join_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
                try:
                    _lib.check(lib.tsq_join_set_radix(h, abi.RADIX_FORCE), h)
                    _lib.check(lib.tsq_join_set_key_packing(h, abi.RADIX_FORCE), h)
                    ctx.sync()
                    ctx.timer_start()
                    _lib.check(lib.tsq_join_build_push(h, bcols, 2, nb), h)
                    _lib.check(lib.tsq_join_build_finish(h), h)
                    _lib.check(lib.tsq_join_probe_push(h, pcols, 2, npr, None), h)
                    first = ctx.timer_stop_ms()
                    again = float("nan")
                    for _ in range(passes - 1):
                        ctx.timer_start()
                        _lib.check(lib.tsq_join_probe_push(h, pcols, 2, npr, None), h)
                        again = ctx.timer_stop_ms()
                    st = abi.Stats()
                    _lib.check(lib.tsq_join_stats(h, C.byref(st)), h)
                    _lib.check(lib.tsq_join_probe_finish(h), h)
                    c = C.c_int64(0)
                    _lib.check(lib.tsq_join_count(h, C.byref(c)), h)
                    rows = c.value // passes
                    fp = _fingerprint(ctx, h) if fingerprint else None
                    return first, again, st, rows, fp
                finally:
                    lib.tsq_join_destroy(h)

        res = {"n_build": nb, "n_probe": npr, "join": "left_outer_nullable" if outer else "inner"}
        fps = {}
        for name, knob in VARIANTS:  # the output check doubles as the warm-up of each variant
            _, _, st, rows, fp = one(knob, 1, fingerprint=True)
            fps[name] = fp
            res[name] = {"rows": rows, "fingerprint": "%d:%016x:%016x" % fp, "route": st.probe_route, "packed_lds_dup": st.packed_lds_dup, "packed_lds_bits": st.packed_lds_bits,
                         "one_pass_ms": [], "repeat_ms": []}
        res["identical"] = bool(fps["sorted_columns"] == fps["lds_dup"] and fps["lds_dup"][0] == res["lds_dup"]["rows"])
        for _ in range(reps):
            for name, knob in VARIANTS:
                first, again, _, _, _ = one(knob, 2)
                res[name]["one_pass_ms"].append(first)
                res[name]["repeat_ms"].append(again)
        return res
    finally:
        for p in [bk, bv, pk, pv] + bms:
            ctx.free(p)


def _mmm(v):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--sizes", default=",".join(str(s) for s in SIZES))
    ap.add_argument("--reps", type=int, default=7)
    ap.add_argument("--outer-at", type=int, default=100_000_000, help="the size at which LEFT OUTER with nullable payloads runs as well (0: never)")
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    lines = ["J-dup (SURVEY.md 8d): build keys r(i,0) mod N_b/4, N_p = N_b/4 uniform probe keys, (k, v) x (k, v), 4 output columns; radix + packing FORCED",
             "ms: median [min .. max] of %d repetitions, device events; one pass = build_push + build_finish + first probe_push; repeat = a further probe_push" % a.reps,
             "%-12s %-20s %-15s %10s %4s  %-32s %-32s %s" % ("N_b", "join", "variant", "rows", "dup", "one pass ms", "repeated probe pass ms", "fingerprint")]
    results = []
    with _lib.Context(0) as ctx:
        for nb in [int(float(s)) for s in a.sizes.split(",") if s]:
            for outer in ([False, True] if nb == a.outer_at else [False]):
                r = run_size(ctx, nb, a.reps, outer)
                results.append(r)
                for name, _ in VARIANTS:
                    v = r[name]
                    lines.append("%-12d %-20s %-15s %10d %4d  %-32s %-32s %s" % (nb, r["join"], name, v["rows"], v["packed_lds_dup"], _mmm(v["one_pass_ms"]), _mmm(v["repeat_ms"]), v["fingerprint"]))
                lines.append("%-12d %-20s outputs identical: %s" % (nb, r["join"], r["identical"]))
                print("\n".join(lines[-3:]), flush=True)
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
            f.write(json.dumps(results) + "\n")
    print(json.dumps({"bench": "dup_join", "all_identical": all(r["identical"] for r in results), "sizes": len(results)}))
    return 0 if all(r["identical"] for r in results) else 1


if __name__ == "__main__":
    sys.exit(main())
