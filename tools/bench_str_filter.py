"""A string-valued filter conjunct (toBool's ETString arm: types.StrToInt(s) != 0) over device-resident rows, JIT forced.

Prints one JSON line: ms per call (median of --reps after --warmup) and the fraction of 8 TB/s on the algorithmic bytes — the
offsets read (8 B per row + 8), the string bytes actually read (every byte of these short, all-digit cells) and 1 B of selected[]
per row.  Usage: python tools/bench_str_filter.py [--rows 100000000] [--reps 20] [--warmup 3]"""
import argparse
import ctypes as C
import json
import os
import sys
import time

import numpy as np

sys.path.insert(0, os.path.dirname(os.path.dirname(os.path.abspath(__file__))))

from tinysql_amd import _abi as abi  # noqa: E402
from tinysql_amd import _lib  # noqa: E402
from tinysql_amd import expression as E  # noqa: E402


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", type=int, default=100_000_000)
    ap.add_argument("--reps", type=int, default=20)
    ap.add_argument("--warmup", type=int, default=3)
    a = ap.parse_args()
    n = a.rows
    rng = np.random.default_rng(1)
    # short numeric strings: 1-4 digits with a non-zero first digit, and a fifth of them "0" (the rows the filter drops)
    zero = rng.random(n) < 0.2
    lens = rng.integers(1, 5, n).astype(np.int64)
    lens[zero] = 1
    offs = np.zeros(n + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    nbytes = int(offs[-1])
    data = (rng.integers(0, 10, nbytes) + 48).astype(np.uint8)
    data[offs[:-1]] = (rng.integers(1, 10, n) + 48).astype(np.uint8)
    data[offs[:-1][zero]] = 48
    with _lib.Context(0) as ctx:
        dd, do, flags = ctx.alloc(nbytes + 64), ctx.alloc(8 * (n + 1) + 64), ctx.alloc(n + 64)
        try:
            ctx.h2d(dd, data)
            ctx.h2d(do, offs)
            col = (abi.Col * 1)()
            col[0].data, col[0].offsets, col[0].length, col[0].elem_size, col[0].type, col[0].flags = dd, do, n, -1, abi.BYTES, abi.COL_DEVICE
            ce = E.CompiledExpr(ctx, [E.Column(0, abi.BYTES)], jit=abi.JIT_FORCE)
            w = C.c_int64(0)
            times = []
            for r in range(a.warmup + a.reps):
                _lib.check(ctx.lib.tsq_ctx_sync(ctx.h), ctx.h)
                t0 = time.perf_counter()
                _lib.check(ctx.lib.tsq_filter_eval(ce.h, col, 1, n, None, flags, None, C.byref(w)), ce.h)
                _lib.check(ctx.lib.tsq_ctx_sync(ctx.h), ctx.h)
                if r >= a.warmup:
                    times.append((time.perf_counter() - t0) * 1e3)
            out = np.zeros(n, np.uint8)
            ctx.d2h(out, flags)
            assert int(out.sum()) == int((~zero).sum()), "selected rows differ from the non-zero strings"
            jl = ce.jit_launches()
            ce.close()
        finally:
            for p in (dd, do, flags):
                ctx.free(p)
    ms = float(np.median(times))
    algo = 8 * (n + 1) + nbytes + n
    print(json.dumps({"bench": "str_filter", "rows": n, "ms": round(ms, 4), "ms_min": round(min(times), 4), "algo_bytes": algo,
                      "frac_of_8TBps": round(algo / (ms * 1e-3) / 8e12, 4), "jit_launches": jl, "reps": a.reps}))


if __name__ == "__main__":
    main()
