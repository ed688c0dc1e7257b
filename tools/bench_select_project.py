#!/usr/bin/env python3
"""A/B of SELECT e1, .., em FROM t WHERE f1 AND .. AND fk on device-resident columns: the separate operators (tsq_filter_eval +
tsq_chunk_compact + one tsq_expr_eval per computed output: what GpuProjectionExec over GpuSelectionExec issue) against the fused
operator (tsq_project_run, csrc/tsq_project.h).  The separate leg uses only calls older libraries have too, so this file can be run
on a build of the commit before the fused operator: the fused leg is skipped when the library lacks tsq_project_create.

Workload: --rows rows (default 1e8) generated in HBM (tsq_gen_column), BIGINT a, b and DOUBLE c uniform in [0, 1):
  sel_1pct   WHERE a < b AND c > 0.98   a, b uniform in [0, 1000)   outputs (a + b) * 3 - a, a - b, c
  sel_50pct  WHERE a < b AND c > 0.5    a = 0, b uniform in [0, 2^40)
  sel_100pct WHERE a < b AND c > -1.0   a = 0, b uniform in [0, 2^40)
  no_filter  (no WHERE)                 a, b uniform in [0, 1000)   outputs a + b, a - b, a * b, (a + b) * 3 - a
(the threshold on c moves with the shape: the generator's doubles are uniform in [0, 1)).  A bare column costs the separate leg
nothing after the compaction (GpuProjectionExec hands the child's column on); the fused leg writes it as an output.
Both legs run with the specialised kernels (TSQ_JIT_FORCE), compiled by one warm-up pass; then --reps timed passes, device events on
the context's stream around the whole sequence of calls (tsq_timer_start / tsq_timer_stop_ms): median [min .. max].  The fused leg
also reports the device time of its evaluate-and-scatter kernel alone, its algorithmic bytes (8 N per filter column + 1 N flags
written + 2 N flags read + 8 B per selected cell of each column the outputs read + 8 m n_out written) and what fraction of 8 TB/s
they are over the fused pass.
   python tools/bench_select_project.py [--rows 1e8] [--reps 5] [--out FILE]"""
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

F, K = E.ScalarFunction, E.Constant
A, B, Cc = E.Column(0, abi.I64), E.Column(1, abi.I64), E.Column(2, abi.F64)
O_MIX = F("minus", F("mul", F("plus", A, B), K(3)), A)
HBM_BYTES_PER_MS = 8e12 / 1e3

# name, (modulus of a, modulus of b), threshold on c or None = no filter, outputs, distinct columns the outputs read
SHAPES = [
    ("sel_1pct", (1000, 1000), 0.98, [O_MIX, F("minus", A, B), Cc], 3),
    ("sel_50pct", (1, 1 << 40), 0.5, [O_MIX, F("minus", A, B), Cc], 3),
    ("sel_100pct", (1, 1 << 40), -1.0, [O_MIX, F("minus", A, B), Cc], 3),
    ("no_filter", (1000, 1000), None, [F("plus", A, B), F("minus", A, B), F("mul", A, B), O_MIX], 2),
]


def spec(kind, col, m=0):
    s = abi.GenSpec()
    s.kind, s.table, s.col, s.seed, s.m = kind, 9, col, 42, m
    return s


class Table:
    """a, b, c in HBM"""

    def __init__(self, ctx, n, ma, mb):
        self.ctx, self.n = ctx, n
        self.ptr = [ctx.alloc(n * 8 + 64) for _ in range(3)]
        ctx.gen_column(spec(abi.GEN_RAND_MOD, 0, ma), n, self.ptr[0])
        ctx.gen_column(spec(abi.GEN_RAND_MOD, 1, mb), n, self.ptr[1])
        ctx.gen_column(spec(abi.GEN_RAND_F64, 2), n, self.ptr[2])
        self.cols = dev_cols(self.ptr, [abi.I64, abi.I64, abi.F64], n)

    def free(self):
        for p in self.ptr:
            self.ctx.free(p)


def dev_cols(ptrs, types, n, bitmaps=None):
    c = (abi.Col * len(ptrs))()
    for i, (p, t) in enumerate(zip(ptrs, types)):
        c[i].data, c[i].length, c[i].elem_size, c[i].type, c[i].flags = p, n, 8, t, abi.COL_DEVICE
        if bitmaps:
            c[i].null_bitmap = bitmaps[i]
    return c


def filters_of(thr):
    return [] if thr is None else [F("lt", A, B), F("gt", Cc, K(float(thr)))]


def separate_leg(ctx, tab, filters, outputs, reps):
    lib, n = ctx.lib, tab.n
    computed = [e for e in outputs if not isinstance(e, E.Column)]
    fe = E.CompiledExpr(ctx, filters, jit=abi.JIT_FORCE) if filters else None
    ces = [E.CompiledExpr(ctx, [e], jit=abi.JIT_FORCE) for e in computed]
    flags = ctx.alloc(n + 64)
    cdata = [ctx.alloc(n * 8 + 64) for _ in range(3)] if filters else []
    odata = [(ctx.alloc(n * 8 + 64), ctx.alloc(n // 8 + 64)) for _ in computed]
    ms, n_out = [], n
    try:
        for it in range(reps + 1):
            ctx.sync()
            ctx.timer_start()
            cols, m = tab.cols, C.c_int64(n)
            if filters:
                w = C.c_int64(0)
                _lib.check(lib.tsq_filter_eval(fe.h, tab.cols, 3, n, None, flags, None, C.byref(w)), fe.h)
                cols = dev_cols(cdata, [abi.I64, abi.I64, abi.F64], n)
                _lib.check(lib.tsq_chunk_compact(ctx.h, tab.cols, 3, n, flags, cols, C.byref(m)), ctx.h)
                for i in range(3):
                    cols[i].length = m.value
            for ce, (d, bm) in zip(ces, odata):
                if m.value == 0:
                    break
                oc = dev_cols([d], [abi.F64 if ce.exprs[0].eval_type == E.ETReal else abi.I64], m.value, [bm])
                w = C.c_int64(0)
                _lib.check(lib.tsq_expr_eval(ce.h, cols, 3, m.value, None, oc, C.byref(w)), ce.h)
            t = ctx.timer_stop_ms()
            n_out = m.value
            if it:
                ms.append(t)
        return ms, n_out
    finally:
        for ce in ces + ([fe] if fe else []):
            ce.close()
        for p in [flags] + cdata + [x for pair in odata for x in pair]:
            ctx.free(p)


def fused_leg(ctx, tab, filters, outputs, reps):
    lib, n = ctx.lib, tab.n
    fp, op = E.compile_list(filters), E.compile_list(outputs)
    h = C.c_void_p()
    _lib.check(lib.tsq_project_create(ctx.h, fp if filters else None, len(filters), op, len(outputs), C.byref(h)), ctx.h)
    ms, kms, n_out = [], [], 0
    try:
        _lib.check(lib.tsq_project_set_jit(h, abi.JIT_FORCE), h)
        for it in range(reps + 1):
            oc = (abi.Col * len(outputs))()
            m, w = C.c_int64(0), C.c_int64(0)
            ctx.sync()
            ctx.timer_start()
            _lib.check(lib.tsq_project_run(h, tab.cols, 3, n, oc, len(outputs), C.byref(m), C.byref(w)), h)
            t = ctx.timer_stop_ms()
            ev, jl, k = C.c_int64(0), C.c_int64(0), C.c_double(0)
            _lib.check(lib.tsq_project_stats(h, C.byref(ev), C.byref(jl), C.byref(k)), h)
            n_out = m.value
            if it:
                ms.append(t)
                kms.append(k.value)
        return ms, kms, n_out, jl.value == ev.value
    finally:
        lib.tsq_project_destroy(h)


def _mmm(v):
    return "%8.3f [%8.3f .. %8.3f]" % (float(np.median(v)), min(v), max(v))


def main():
    ap = argparse.ArgumentParser()
    ap.add_argument("--rows", default="1e8")
    ap.add_argument("--reps", type=int, default=5)
    ap.add_argument("--shapes", default=",".join(s[0] for s in SHAPES))
    ap.add_argument("--out", default=None)
    a = ap.parse_args()
    n = int(float(a.rows))
    results = []
    lines = ["%d device-resident rows; ms per pass: median [min .. max] of %d repetitions after one warm-up pass, device events; TSQ_JIT_FORCE" % (n, a.reps),
             "%-11s %-9s %12s  %-32s %s" % ("shape", "leg", "rows out", "ms", "fused only: kernel ms, algorithmic MB, fraction of 8 TB/s over the pass")]
    with _lib.Context(0) as ctx:
        fused = hasattr(ctx.lib, "tsq_project_create")
        for name, (ma, mb), thr, outputs, n_read in SHAPES:
            if name not in a.shapes.split(","):
                continue
            tab = Table(ctx, n, ma, mb)
            try:
                filters = filters_of(thr)
                r = {"shape": name, "rows": n}
                ms, n_out = separate_leg(ctx, tab, filters, outputs, a.reps)
                r["separate_ms"], r["rows_out"] = ms, n_out
                lines.append("%-11s %-9s %12d  %-32s" % (name, "separate", n_out, _mmm(ms)))
                if fused:
                    ms, kms, n_out2, jit_ok = fused_leg(ctx, tab, filters, outputs, a.reps)
                    nbytes = (8 * 3 * n + 3 * n if filters else 0) + 8 * n_read * n_out2 + 8 * len(outputs) * n_out2
                    r.update({"fused_ms": ms, "fused_kernel_ms": kms, "fused_rows_out": n_out2, "fused_jit": jit_ok, "algorithmic_bytes": nbytes})
                    lines.append("%-11s %-9s %12d  %-32s %8.3f  %9.1f  %.3f%s" % (name, "fused", n_out2, _mmm(ms), float(np.median(kms)), nbytes / 1e6,
                                                                                    nbytes / (float(np.median(ms)) * HBM_BYTES_PER_MS),
                                                                                    "" if jit_ok and n_out2 == n_out else "  (!) rows differ or the interpreter served"))
                results.append(r)
                print("\n".join(lines[-2:] if fused else lines[-1:]), flush=True)
            finally:
                tab.free()
    text = "\n".join(lines) + "\n"
    if a.out:
        with open(a.out, "w") as f:
            f.write(text)
            f.write(json.dumps(results) + "\n")
    print(json.dumps({"bench": "select_project", "fused_leg": fused, "cases": len(results)}))
    return 0


if __name__ == "__main__":
    sys.exit(main())
