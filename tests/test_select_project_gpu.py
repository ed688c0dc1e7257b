"""GPU: the fused Selection + Projection operator (tsq_project_*, ABI 10) through the C-ABI on device chunks, against the CPU oracle
chained the way the reference chains ProjectionExec over SelectionExec: orc.filter_eval gives the selected rows, boolean indexing
keeps them, orc.expr_eval / orc.expr_eval_str runs per output.  Everything is compared in order and bit for bit (the arithmetic per
row is the code of tsq_expr_eval: no tolerance): n_out, values where NOT NULL, null flags, offsets and bytes of string outputs, the
division-by-zero count and the status code."""
import ctypes as C
import os
import sys

import numpy as np
import pytest

from oracle import binding as orc
from tests import strtoint_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd import gpu_pipeline as GP
from tinysql_amd.chunk import Chunk, Column, StrColumn, unpack_bitmap

pytestmark = pytest.mark.gpu

F, K = E.ScalarFunction, E.Constant
C0, C1, C2, C3, C4 = E.Column(0, abi.I64), E.Column(1, abi.I64), E.Column(2, abi.F64), E.Column(3, abi.F32), E.Column(4, abi.U64)
JITS = [abi.JIT_OFF, abi.JIT_FORCE]
IMAX = (1 << 63) - 1

FILTERS = [F("lt", C0, C1), F("gt", C2, K(0.5))]
OUTPUTS = [
    F("minus", F("mul", F("plus", C0, C1), K(3)), C0),
    F("mul", C2, F("minus", K(1.0), C3)),
    F("div", C2, C3),                                   # zero divisors: NULL + a warning
    F("if", F("gt", C0, K(0)), C1, F("ifnull", C0, C1)),
    F("plus", C4, C4),                                  # TSQ_F_*_UNSIGNED
    C1,
    C3,                                                 # a bare F32 column is widened
]


def main_chunk(n, seed=None):
    """nullable I64, I64, nullable F64, nullable F32, U64; row 0 always passes FILTERS"""
    rng = np.random.default_rng(n if seed is None else seed)
    c0, c1 = rng.integers(-50, 50, n), rng.integers(-50, 50, n)
    c2 = rng.random(n)
    c3 = rng.choice(np.array([0.0, 0.0, 0.25, 0.5, 1.5, -2.0], np.float32), n)
    nn0, nn2, nn3 = rng.random(n) > 0.1, rng.random(n) > 0.1, rng.random(n) > 0.15
    c0[0], c1[0], c2[0], nn0[0], nn2[0] = -1, 5, 0.75, True, True
    return Chunk([Column(abi.I64, c0, nn0), Column(abi.I64, c1), Column(abi.F64, c2, nn2), Column(abi.F32, c3, nn3),
                  Column(abi.U64, rng.integers(0, 1 << 62, n).astype(np.uint64))])


def take(chk, sel):
    cols = []
    for c in chk.columns:
        if c.tp == abi.BYTES:
            cols.append(StrColumn([v for v, k in zip(c.values(), sel) if k]))
        else:
            cols.append(Column(c.tp, c.data[sel], None if c.notnull is None else c.notnull[sel]))
    return Chunk(cols)


def oracle_chain(chk, filters, outputs, str_ctx=0):
    """(status, n_out, [per output: (data, notnull) or (offsets, bytes, notnull)], div0 warnings)"""
    w = 0
    try:
        kept = chk
        if filters:
            sel, _, wf = orc.filter_eval(E.compile_list(filters, str_ctx), len(filters), chk)
            w += wf
            kept = take(chk, sel)
        cols = []
        if kept.NumRows() == 0:
            return abi.OK, 0, [], w
        for e in outputs:  # defaultEvaluator.run: the first failing expression ends the statement
            prog = E.compile_expr(e, str_ctx)
            if prog.result_type == abi.BYTES:
                offs, data, nn, wo = orc.expr_eval_str(prog, kept)
                cols.append((offs, data, nn))
            else:
                col, wo = orc.expr_eval(prog, kept)
                cols.append((col.data, np.ones(len(col.data), bool) if col.notnull is None else col.notnull))
            w += wo
        return abi.OK, kept.NumRows(), cols, w
    except orc.OracleError as ex:
        return ex.status, 0, [], w


class Project:
    """a tsq_project handle"""

    def __init__(self, ctx, filters, outputs, jit, str_ctx=0):
        self.ctx, self.lib, self.m = ctx, ctx.lib, len(outputs)
        self.fp, self.op = E.compile_list(filters, str_ctx), E.compile_list(outputs, str_ctx)
        h = C.c_void_p()
        _lib.check(self.lib.tsq_project_create(ctx.h, self.fp if filters else None, len(filters), self.op, len(outputs), C.byref(h)), ctx.h)
        self.h = h
        _lib.check(self.lib.tsq_project_set_jit(h, jit), h)

    def run(self, dev):
        """(status, n_out, host copies of the borrowed outputs, div0 warnings)"""
        oc = (abi.Col * self.m)()
        m, w = C.c_int64(-1), C.c_int64(-1)
        st = self.lib.tsq_project_run(self.h, dev.cols(), len(dev.columns), dev.nrows, oc, self.m, C.byref(m), C.byref(w))
        if st != abi.OK:
            return st, 0, [], w.value
        n = m.value
        cols = []
        for j, c in enumerate(oc):
            assert c.length == n and c.flags & abi.COL_DEVICE and c.flags & abi.COL_BORROW
            if n == 0:
                continue
            bm = np.zeros((n + 7) // 8, np.uint8)
            self.ctx.d2h(bm, c.null_bitmap)
            nn = unpack_bitmap(bm, n)
            if c.type == abi.BYTES:
                assert c.elem_size == -1
                offs = np.zeros(n + 1, np.int64)
                self.ctx.d2h(offs, c.offsets)
                data = np.zeros(int(offs[n]), np.uint8)
                if offs[n]:
                    self.ctx.d2h(data, c.data)
                cols.append((offs, data, nn))
            else:
                assert c.elem_size == 8 and c.type == (abi.F64 if self.op[j].result_type == abi.F64 else (abi.U64 if self.op[j].result_unsigned else abi.I64))
                data = np.zeros(n, np.uint64)
                self.ctx.d2h(data, c.data)
                cols.append((data, nn))
        return st, n, cols, w.value

    def stats(self):
        a, b, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_project_stats(self.h, C.byref(a), C.byref(b), C.byref(ms)), self.h)
        return a.value, b.value, ms.value

    def str_warnings(self):
        t, o = C.c_int64(-1), C.c_int64(-1)
        assert self.lib.tsq_project_str_warnings(self.h, C.byref(t), C.byref(o)) == abi.OK
        return t.value, o.value

    def message(self):
        return (self.lib.tsq_last_error(self.h) or b"").decode(errors="replace")

    def close(self):
        self.lib.tsq_project_destroy(self.h)
        self.h = None


def same(got, want):
    print("status %d/%d n_out %d/%d div0 %d/%d" % (got[0], want[0], got[1], want[1], got[3], want[3]))
    assert got[0] == want[0], ("status", got[0], want[0])
    if want[0] != abi.OK:
        return
    assert got[1] == want[1], ("n_out", got[1], want[1])
    assert got[3] == want[3], ("division-by-zero warnings", got[3], want[3])
    assert len(got[2]) == len(want[2])
    for j, (g, w) in enumerate(zip(got[2], want[2])):
        assert np.array_equal(g[-1], w[-1]), ("null flags of output", j)
        if len(w) == 3:
            assert np.array_equal(g[0], w[0]), ("offsets of output", j)
            assert g[1].tobytes() == w[1].tobytes(), ("bytes of output", j)
        else:
            nn = w[-1]
            assert np.array_equal(np.ascontiguousarray(g[0]).view(np.uint64)[nn], np.ascontiguousarray(w[0]).view(np.uint64)[nn]), ("values of output", j)


def check(ctx, chk, filters, outputs, jit, want=None, str_ctx=0, launches=None):
    """launches: the evaluate-and-scatter launches this run must make (default: one iff the oracle selects a row and raises no error)"""
    want = want or oracle_chain(chk, filters, outputs, str_ctx)
    dev = GP.DeviceChunk.from_host(ctx, chk)
    p = Project(ctx, filters, outputs, jit, str_ctx)
    try:
        got = p.run(dev)
        same(got, want)
        ev, jl, _ = p.stats()
        assert ev == ((1 if want[0] == abi.OK and want[1] > 0 else 0) if launches is None else launches)
        if jit == abi.JIT_FORCE and ev:
            assert jl == ev, p.message()  # the specialised kernel ran (a hiprtc failure would fall back to the interpreter silently)
        return got, p.message()
    finally:
        p.close()
        dev.free()


_want = {}


def main_case(n):
    if n not in _want:
        chk = main_chunk(n)
        _want[n] = (chk, oracle_chain(chk, FILTERS, OUTPUTS))
    return _want[n]


@pytest.mark.parametrize("jit", JITS)
@pytest.mark.parametrize("n", [1, 63, 64, 65, 257, 4096, 70001])
def test_filter_and_seven_outputs_equal_the_oracle_chain(ctx, n, jit):
    chk, want = main_case(n)
    assert want[0] == abi.OK and want[1] >= 1 and (n < 4096 or (want[3] > 0 and 0.1 * n < want[1] < 0.4 * n))
    check(ctx, chk, FILTERS, OUTPUTS, jit, want)


@pytest.mark.parametrize("jit", JITS)
def test_selectivity_edges(ctx, jit):
    n = 1000
    chk = main_chunk(n)
    none = [F("lt", C1, K(-1000))]
    every = [F("ge", C1, K(-1000))]
    assert check(ctx, chk, none, OUTPUTS, jit)[0][1] == 0
    assert check(ctx, chk, every, OUTPUTS, jit)[0][1] == n
    # rows dropped only because a conjunct is NULL: c0 = c0 is true for every NOT NULL row
    got = check(ctx, chk, [F("eq", C0, C0)], OUTPUTS, jit)[0]
    assert 0 < got[1] == int(chk.columns[0].notnull.sum()) < n


@pytest.mark.parametrize("jit", JITS)
@pytest.mark.parametrize("which", ["with_an_f32_column", "eight_byte_columns"])  # the second takes the specialised form's four-row loop
@pytest.mark.parametrize("n", [1, 257, 4096, 70001])
def test_without_filters_it_is_tsq_expr_eval_per_expression(ctx, n, jit, which):
    chk = main_chunk(n, seed=7 * n)
    outs = OUTPUTS[:4] if which == "with_an_f32_column" else [OUTPUTS[0], OUTPUTS[3], OUTPUTS[4], F("div", C2, F("minus", C2, K(0.25)))]
    want_cols, w = [], 0
    for e in outs:  # the separate operator, on the same chunk
        ce = E.CompiledExpr(ctx, [e], jit=jit)
        try:
            col = ce.VecEval(chk)
            want_cols.append((col.data, np.ones(n, bool) if col.notnull is None else col.notnull))
            w += ce.warnings
        finally:
            ce.close()
    dev = GP.DeviceChunk.from_host(ctx, chk)
    p = Project(ctx, [], outs, jit)
    try:
        same(p.run(dev), (abi.OK, n, want_cols, w))
        assert p.stats()[0] == 1  # one launch for four outputs
        same(p.run(dev), (abi.OK, n, want_cols, w))
        assert p.stats()[:2] == (2, 2 if jit == abi.JIT_FORCE else 0)
    finally:
        p.close()
        dev.free()
    same((abi.OK, n, want_cols, w), oracle_chain(chk, [], outs))


def overflow_chunk(n=3000):
    """c0 + c1 overflows BIGINT exactly on the rows with c4 == 1 (none of them passes c4 = 0)"""
    rng = np.random.default_rng(5)
    bad = rng.random(n) < 0.3
    bad[n - 1] = True
    c0 = np.where(bad, IMAX - 3, rng.integers(-50, 50, n))
    c1 = np.where(bad, 100, rng.integers(-50, 50, n))
    c2 = np.where(bad, 1.5e308, rng.random(n))
    return Chunk([Column(abi.I64, c0), Column(abi.I64, c1), Column(abi.F64, c2), Column(abi.F32, np.ones(n, np.float32)), Column(abi.U64, bad.astype(np.uint64))]), bad


@pytest.mark.parametrize("jit", JITS)
def test_errors_come_from_selected_rows_only(ctx, jit):
    chk, bad = overflow_chunk()
    n = chk.NumRows()
    add, dbl = F("plus", C0, C1), F("mul", C2, K(10.0))
    good = [F("eq", C4, K(0, unsigned=True))]
    got, _ = check(ctx, chk, good, [add, C1], jit)
    assert got[0] == abi.OK and got[1] == int((~bad).sum())
    # the filter widened by ONE overflowing row (the last row of the chunk)
    c5 = Column(abi.I64, (np.arange(n) == n - 1).astype(np.int64))
    chk6 = Chunk(chk.columns + [c5])
    wide = [F("or", F("eq", C4, K(0, unsigned=True)), F("eq", E.Column(5, abi.I64), K(1)))]
    got, msg = check(ctx, chk6, wide, [add, C1], jit, launches=1)
    assert got[0] == abi.ERR_OVERFLOW_BIGINT and "output 0" in msg and "row %d" % (n - 1) in msg
    # output 0 raises a DOUBLE overflow, output 1 a BIGINT overflow: the first failing expression is the statement's error
    got, msg = check(ctx, chk6, wide, [dbl, add], jit, launches=1)
    assert got[0] == abi.ERR_OVERFLOW_DOUBLE and "output 0" in msg
    got, msg = check(ctx, chk6, wide, [add, dbl], jit, launches=1)
    assert got[0] == abi.ERR_OVERFLOW_BIGINT and "output 0" in msg
    got, msg = check(ctx, chk6, wide, [C1, dbl, add], jit, launches=1)
    assert got[0] == abi.ERR_OVERFLOW_DOUBLE and "output 1" in msg
    # a filter that itself overflows: its error wins and no output is evaluated
    got, msg = check(ctx, chk, [F("gt", add, K(0))], [dbl], jit, launches=0)
    assert got[0] == abi.ERR_OVERFLOW_BIGINT and "filter" in msg


@pytest.mark.parametrize("jit", JITS)
def test_division_by_zero_is_counted_over_selected_rows_only(ctx, jit):
    n = 5000
    chk = main_chunk(n, seed=99)
    c2, c3 = chk.columns[2], chk.columns[3]
    # a filter that divides (c2 / c3 > 0.1: x / 0 is NULL, the row is dropped, the warning counted) and two dividing outputs
    filters = [F("gt", F("div", C2, C3), K(0.1)), F("lt", C0, C1)]
    outs = [F("div", C2, F("minus", C3, K(1.5))), F("div", K(1.0), F("minus", C2, C2))]
    want = oracle_chain(chk, filters, outs)
    zero_div_all = int((c2.notnull & c3.notnull & (c3.data == 0)).sum())
    assert want[0] == abi.OK and want[1] > 100 and want[3] > zero_div_all + want[1]  # filter's + (some of output 0) + every row of output 1
    check(ctx, chk, filters, outs, jit, want)
    # the same outputs without the filter count every row: strictly more
    assert oracle_chain(chk, [], outs)[3] > want[3]


def string_chunk(n, maxlen, seed):
    rng = np.random.default_rng(seed)
    alphabet = np.frombuffer(b"abcxyz0189 -", np.uint8)

    def cells(null_frac):
        out = []
        for ln, isnull in zip(rng.integers(0, maxlen + 1, n), rng.random(n) < null_frac):
            out.append(None if isnull else rng.choice(alphabet, ln).tobytes())
        return out
    s0, s1 = cells(0.1), cells(0.05)
    for i in range(0, n, 7):  # equal cells for the EQ_STR conjunct
        s1[i] = s0[i]
    return Chunk([StrColumn(s0), StrColumn(s1), Column(abi.I64, rng.integers(-3, 4, n), rng.random(n) > 0.1)])


S0, S1, I2 = E.Column(0, abi.BYTES), E.Column(1, abi.BYTES), E.Column(2, abi.I64)


@pytest.mark.parametrize("jit", JITS)
@pytest.mark.parametrize("maxlen", [8, 200], ids=["cells_0_8_bytes", "cells_0_200_bytes"])
def test_string_outputs_and_an_eq_str_conjunct(ctx, maxlen, jit):
    chk = string_chunk(1000, maxlen, maxlen)
    outs = [S0, F("if", F("gt", I2, K(0)), S0, S1), K("const!"), F("plus", I2, K(1)), F("ifnull", S0, K("(null)"))]
    for filters in ([F("gt", I2, K(-2))], [F("eq", S0, S1)], []):
        want = oracle_chain(chk, filters, outs)
        assert want[0] == abi.OK and want[1] > 50
        check(ctx, chk, filters, outs, jit, want)
    long_copy = sum(len(v) for v in chk.columns[0].values() if v) / 1000 > 32
    assert long_copy == (maxlen == 200)  # one cell per wave for the long cells, one per lane for the short ones


@pytest.mark.parametrize("jit", JITS)
def test_a_string_valued_conjunct_and_its_warnings(ctx, jit):
    from tests.test_filter_string_gpu import expr_of, mk_chunk, model, vocab
    ok = [s for s in vocab() if not R.str_to_int(s, R.CTX_SELECT)[1] & (R.ERR_OVF | R.ERR_TRUNC)]
    chk = mk_chunk(41, 1000, ok)  # string, string, I64, F64
    conjs = [("int", -2), ("s0", None)]
    sel, _, trunc, ovf, st = model(chk, conjs, R.CTX_SELECT)
    assert st == abi.OK and 0 < sel.sum() < 1000 and trunc > 0
    kept = take(chk, sel)
    outs = [E.Column(1, abi.BYTES), E.Column(2, abi.I64), E.Column(3, abi.F64)]
    want_cols = []
    for e in outs:
        prog = E.compile_expr(e)
        if prog.result_type == abi.BYTES:
            want_cols.append(orc.expr_eval_str(prog, kept)[:3])
        else:
            col = orc.expr_eval(prog, kept)[0]
            want_cols.append((col.data, np.ones(len(col.data), bool) if col.notnull is None else col.notnull))
    dev = GP.DeviceChunk.from_host(ctx, chk)
    p = Project(ctx, [expr_of(k, a) for k, a in conjs], outs, jit, str_ctx=R.CTX_SELECT)
    try:
        same(p.run(dev), (abi.OK, int(sel.sum()), want_cols, 0))
        assert p.str_warnings() == (trunc, ovf)
    finally:
        p.close()
        dev.free()
    # the conjunct's own error (the last non-NULL row that reached it overflows) is the run's, with the filter's warnings
    bad = Chunk([StrColumn(chk.columns[0].values()[:-1] + [b"99999999999999999999"]), chk.columns[1], Column(abi.I64, np.ones(1000, np.int64)), chk.columns[3]])
    want = model(bad, conjs, R.CTX_SELECT)
    assert want[4] == abi.ERR_OVERFLOW_BIGINT
    dev = GP.DeviceChunk.from_host(ctx, bad)
    p = Project(ctx, [expr_of(k, a) for k, a in conjs], outs, jit, str_ctx=R.CTX_SELECT)
    try:
        assert p.run(dev)[0] == abi.ERR_OVERFLOW_BIGINT and "filter" in p.message()
        assert p.str_warnings() == (want[2], want[3]) and p.stats()[0] == 0
    finally:
        p.close()
        dev.free()


@pytest.mark.parametrize("jit", JITS)
def test_one_handle_over_chunks_of_different_sizes(ctx, jit):
    p = Project(ctx, FILTERS, OUTPUTS, jit)
    devs = []
    try:
        for n in (70001, 64, 5000, 70001):
            chk, want = main_case(n) if n != 5000 else (main_chunk(5000), None)
            want = want or oracle_chain(chk, FILTERS, OUTPUTS)
            dev = GP.DeviceChunk.from_host(ctx, chk)
            devs.append(dev)
            same(p.run(dev), want)
        assert p.stats()[0] == 4
        # an empty chunk and a chunk without a selected row leave outputs of length 0
        st, n_out, _, w = p.run(GP.DeviceChunk(devs[0].columns, 0))
        assert (st, n_out, w) == (abi.OK, 0, 0) and p.stats()[0] == 4
    finally:
        p.close()
        for d in devs:
            d.free()


def test_refusals(ctx):
    lib = ctx.lib
    progs = E.compile_list(OUTPUTS[:1] * 17)
    h = C.c_void_p()
    for nf, no in ((0, 0), (0, 17), (17, 1)):
        assert lib.tsq_project_create(ctx.h, progs, nf, progs, no, C.byref(h)) == abi.ERR_INVALID and not h.value
        assert ("n_outputs" if nf == 0 else "n_filters") in _lib.last_error(ctx.h)
    chk = main_chunk(100)
    p = Project(ctx, FILTERS, OUTPUTS[:2], abi.JIT_OFF)
    dev = GP.DeviceChunk.from_host(ctx, chk)
    try:
        keep = []
        from tinysql_amd.chunk import make_cols
        oc = (abi.Col * 2)()
        m = C.c_int64(0)
        assert lib.tsq_project_run(p.h, make_cols(chk.columns, keep), 5, 100, oc, 2, C.byref(m), None) == abi.ERR_INVALID  # host-resident columns
        assert "device resident" in p.message()
        assert lib.tsq_project_run(p.h, dev.cols(), 5, 100, oc, 3, C.byref(m), None) == abi.ERR_INVALID  # n_out_cols != the outputs
        # a program that references a column the chunk does not have: the validator's error
        assert lib.tsq_project_run(p.h, dev.cols(), 2, 100, oc, 2, C.byref(m), None) == abi.ERR_INVALID
        assert "column index out of range" in p.message()
        assert p.run(dev)[0] == abi.OK  # the handle is still good
    finally:
        p.close()
        dev.free()
    with pytest.raises(E.Unsupported):  # the operator refuses at construction what the library refuses
        GP.GpuSelectProjectExec(ctx, GP.DeviceTableScan(ctx, dev), [], [])


@pytest.mark.parametrize("jit", JITS)
def test_pipeline_operator_equals_projection_over_selection(ctx, jit):
    sys.path.insert(0, os.path.join(os.path.dirname(os.path.dirname(os.path.abspath(__file__))), "tools"))
    import q3
    lineitem = q3.tables(0.05)[2]  # orderkey, shipdate, extendedprice, discount: 3e5 rows
    I, D = abi.I64, abi.F64
    filt = [F("gt", E.Column(1, I), K(q3.D)), F("lt", E.Column(3, D), K(0.07))]
    exprs = [E.Column(0, I), F("mul", E.Column(2, D), F("minus", K(1.0), E.Column(3, D))), F("plus", E.Column(0, I), E.Column(1, I)), E.Column(3, D)]
    dev = GP.DeviceChunk.from_host(ctx, lineitem)
    try:
        fused = GP.GpuSelectProjectExec(ctx, GP.DeviceTableScan(ctx, dev, batch_rows=50_000), filt, exprs, jit=jit)
        assert fused.Schema() == [I, D, I, D]
        got = GP.drain_device(fused)
        want = GP.drain_device(GP.GpuProjectionExec(ctx, GP.GpuSelectionExec(ctx, GP.DeviceTableScan(ctx, dev, batch_rows=50_000), filt, jit=jit), exprs, jit=jit))
        assert len(got) == len(want) > 1 and sum(c.NumRows() for c in got) > 10_000
        for g, w in zip(got, want):
            assert g.types() == w.types() and g.NumRows() == w.NumRows()
            for gc, wc in zip(g.columns, w.columns):
                gn = np.ones(len(gc), bool) if gc.notnull is None else gc.notnull
                wn = np.ones(len(wc), bool) if wc.notnull is None else wc.notnull
                assert np.array_equal(gn, wn) and np.array_equal(gc.data.view(np.uint64)[gn], wc.data.view(np.uint64)[wn])
    finally:
        dev.free()
