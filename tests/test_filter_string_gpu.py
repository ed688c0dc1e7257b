"""GPU: string-valued conjuncts in tsq_filter_eval (toBool's ETString arm, expression/expression.go:281-326, ABI 8) against a numpy
restatement of VecEvalBool over the Python types.StrToInt of tests/strtoint_ref.py: selected[] and nulls[] identical, the warning
counts exact, and the statement error of the last non-NULL row that reached a string conjunct."""
import ctypes as C

import numpy as np
import pytest

from tests import gpu_helpers as G
from tests import strtoint_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column, StrColumn

pytestmark = pytest.mark.gpu

S0, S1, I2, R3 = E.Column(0, abi.BYTES), E.Column(1, abi.BYTES), E.Column(2, abi.I64), E.Column(3, abi.F64)
F = E.ScalarFunction

# the string mix: numbers with spaces, signs, dots, exponents and junk tails, as a vocabulary the rows draw from
BASE = [b"0", b"1", b"-1", b"  12  ", b"abc", b"", b" ", b"0.4", b"0.5", b"-0.5", b"1e3", b"1e-1", b"5e-1", b"+999.9999e2", b"12abc", b"1.5x",
        b"125e342", b"1e21", b"9223372036854775808", b"-9223372036854775809", b"99999999999999999999", b"\xc2\xa07\xe3\x80\x80", b"0x1", b".",
        b"-", b"+5", b"1-5e-2", b"00000000000000000000000003", b"1e9223372036854775808", b"\xff1", b"3\x00"]


def vocabulary(seed, n):
    from tests.test_strtoint_cpu import fuzz_strings
    return BASE + fuzz_strings(seed, n - len(BASE))


def mk_chunk(seed, n, vocab, null_frac=0.05):
    rng = np.random.default_rng(seed)
    pick0, pick1 = rng.integers(0, len(vocab), n), rng.integers(0, len(vocab), n)
    nn0, nn1 = rng.random(n) >= null_frac, rng.random(n) >= null_frac
    s0 = [vocab[k] if ok else None for k, ok in zip(pick0, nn0)]
    s1 = [vocab[k] if ok else None for k, ok in zip(pick1, nn1)]
    ints = Column(abi.I64, rng.integers(-3, 4, n), rng.random(n) >= 0.1)
    reals = Column(abi.F64, rng.normal(0, 1.5, n), rng.random(n) >= 0.05)
    return Chunk([StrColumn(s0), StrColumn(s1), ints, reals])


_cache = {}


def s2i_col(cells, mode):
    """(value, flags, notnull) arrays of a list of cells"""
    n = len(cells)
    v, f, nn = np.zeros(n, np.int64), np.zeros(n, np.uint32), np.zeros(n, bool)
    for i, c in enumerate(cells):
        if c is None:
            continue
        k = (c, mode)
        r = _cache.get(k)
        if r is None:
            r = _cache[k] = R.str_to_int(c, mode)
        v[i], f[i], nn[i] = r[0], r[1], True
    return v, f, nn


def model(chk, conjs, mode, sel=None):
    """VecEvalBool (expression.go:205-279) + toBool over the logical rows: (selected, nulls, truncated, overflow, error status)"""
    idx_rows = np.arange(chk.NumRows()) if sel is None else np.asarray(sel)
    cells = [[chk.columns[c]._vals[i] for i in idx_rows] for c in (0, 1)]
    ints = chk.columns[2].data[idx_rows]
    n_all = chk.columns[2].data.shape[0]
    inn = (np.ones(n_all, bool) if chk.columns[2].notnull is None else chk.columns[2].notnull)[idx_rows]
    reals = chk.columns[3].data[idx_rows]
    rnn = (np.ones(n_all, bool) if chk.columns[3].notnull is None else chk.columns[3].notnull)[idx_rows]
    n = len(idx_rows)
    alive, nulls = np.ones(n, bool), np.zeros(n, bool)
    trunc = ovf = 0
    for kind, arg in conjs:
        idx = np.nonzero(alive)[0]
        if kind in ("s0", "s1", "if"):
            if kind == "if":  # IF(i2 > 0, s0, s1)
                take0 = inn & (ints > 0)
                cl = [cells[0][i] if take0[i] else cells[1][i] for i in range(n)]
            else:
                cl = cells[0 if kind == "s0" else 1]
            v, f, nn = s2i_col(cl, mode)
            reached = idx[nn[idx]]
            trunc += int(np.sum(f[reached] & R.TRUNC_WARN))
            ovf += int(np.sum((f[reached] & R.OVF_WARN) >> 1))
            if len(reached) and f[reached[-1]] & (R.ERR_OVF | R.ERR_TRUNC):
                return None, None, trunc, ovf, abi.ERR_OVERFLOW_BIGINT if f[reached[-1]] & R.ERR_OVF else abi.ERR_TRUNCATED_WRONG_VALUE
            alive[idx] = nn[idx] & (v[idx] != 0)
        elif kind == "int":  # i2 > arg: a NULL keeps the row (and marks it)
            nulls[idx[~inn[idx]]] = True
            alive[idx] = ~inn[idx] | (ints[idx] > arg)
        elif kind == "real":  # the bare F64 column: RoundFloat(f) != 0, NULL drops the row
            alive[idx] = rnn[idx] & (np.abs(reals[idx]) >= 0.5)
    return alive & ~nulls, nulls, trunc, ovf, abi.OK


def expr_of(kind, arg):
    if kind == "s0":
        return S0
    if kind == "s1":
        return S1
    if kind == "if":
        return F("if", F("gt", I2, E.Constant(0)), S0, S1)
    if kind == "int":
        return F("gt", I2, E.Constant(arg))
    return R3


def run(ctx, chk, conjs, mode, jit, sel=None, device=False):
    exprs = [expr_of(k, a) for k, a in conjs]
    ce = E.CompiledExpr(ctx, exprs, jit=jit, str_ctx=mode)
    try:
        if not device:
            c = chk if sel is None else Chunk(chk.columns, sel=np.asarray(sel, np.int32))
            try:
                selected, nulls = ce.VectorizedFilter(c, want_nulls=True)
                st = abi.OK
            except _lib.TsqError as ex:
                selected = nulls = None
                st = ex.status
            if jit == abi.JIT_FORCE:
                assert ce.jit_launches() > 0  # the specialised kernel ran (a hiprtc failure would fall back to the interpreter silently)
            return selected, nulls, ce.truncated_warnings, ce.overflow_warnings, st
        n = chk.NumRows()
        dcols = [G.DevStrCol(ctx, chk.columns[0]), G.DevStrCol(ctx, chk.columns[1]), G.to_device(ctx, chk.columns[2]), G.to_device(ctx, chk.columns[3])]
        flags = ctx.alloc(2 * n + 64)
        dsel = None
        try:
            m = n
            if sel is not None:
                m = len(sel)
                dsel = ctx.alloc(4 * m + 64)
                ctx.h2d(dsel, np.asarray(sel, np.int32))
            w = C.c_int64(0)
            st = ctx.lib.tsq_filter_eval(ce.h, G.dev_cols(dcols), 4, m, dsel, flags, flags + n, C.byref(w))
            t, o = C.c_int64(0), C.c_int64(0)
            assert ctx.lib.tsq_expr_str_warnings(ce.h, C.byref(t), C.byref(o)) == abi.OK
            if jit == abi.JIT_FORCE:
                assert ce.jit_launches() > 0
            if st != abi.OK:
                return None, None, t.value, o.value, st
            out = np.zeros(2 * n, np.uint8)
            ctx.d2h(out, flags)
            return out[:m].astype(bool), out[n:n + m].astype(bool), t.value, o.value, st
        finally:
            for d in dcols:
                d.free()
            ctx.free(flags)
            if dsel:
                ctx.free(dsel)
    finally:
        ce.close()


def check(got, want):
    assert got[4] == want[4], (got[4], want[4])
    assert got[2:4] == want[2:4], ("warnings", got[2:4], want[2:4])
    if want[4] == abi.OK:
        assert np.array_equal(got[0], want[0]) and np.array_equal(got[1], want[1])


def safe(chk):
    """the chunk with its last rows made error-free for the string conjuncts (a statement that must succeed): the last 40 rows of both
    string columns (so whichever the IF picks) get "7" """
    n = chk.NumRows()
    s0, s1 = list(chk.columns[0]._vals), list(chk.columns[1]._vals)
    for k in range(n - 40, n):
        s0[k] = s1[k] = b"7"
    return Chunk([StrColumn(s0), StrColumn(s1), chk.columns[2], chk.columns[3]])


VOCAB = None


def vocab():
    global VOCAB
    if VOCAB is None:
        VOCAB = vocabulary(5, 3000)
    return VOCAB


MODES = [R.CTX_SELECT, R.CTX_DELETE, R.CTX_INSERT, R.CTX_OTHER_LOOSE, R.CTX_IGNORE]


@pytest.mark.parametrize("mode", MODES)
@pytest.mark.parametrize("jit", [abi.JIT_OFF, abi.JIT_FORCE])
def test_one_string_conjunct_1e6_rows(ctx, mode, jit):
    chk = safe(mk_chunk(11, 1_000_000, vocab()))
    conjs = [("s0", None)]
    want = model(chk, conjs, mode)
    assert want[4] == abi.OK and want[0].sum() > 1000 and (want[2] > 0 or mode & (R.TRUNCATE_ERROR | R.IGNORE_TRUNCATE))
    check(run(ctx, chk, conjs, mode, jit), want)
    check(run(ctx, chk, conjs, mode, jit, device=True), want)


CNF = [
    [("int", 0), ("s0", None)],
    [("s0", None), ("int", 0)],
    [("real", None), ("s1", None), ("int", -1)],
    [("int", -2), ("if", None), ("real", None), ("s0", None)],
    [("s1", None), ("s0", None)],
    [("if", None)],
]


@pytest.mark.parametrize("k", range(len(CNF)))
@pytest.mark.parametrize("jit", [abi.JIT_OFF, abi.JIT_FORCE])
def test_cnf_lists_mixing_string_int_real(ctx, k, jit):
    conjs = CNF[k]
    chk = safe(mk_chunk(20 + k, 300_000, vocab()))
    rng = np.random.default_rng(k)
    sel = np.sort(rng.permutation(300_000)[:120_000])
    sel = np.concatenate([sel[sel < 299_960], np.arange(299_960, 300_000)])  # the safe tail stays the last logical rows
    for mode in (R.CTX_SELECT, R.CTX_INSERT, R.CTX_IGNORE):
        want = model(chk, conjs, mode)
        check(run(ctx, chk, conjs, mode, jit), want)
        want_sel = model(chk, conjs, mode, sel)
        check(run(ctx, chk, conjs, mode, jit, sel=sel), want_sel)
        check(run(ctx, chk, conjs, mode, jit, sel=sel, device=True), want_sel)


def with_tail(chk, cells0, cells1=None):
    n = chk.NumRows()
    s0, s1 = list(chk.columns[0]._vals), list(chk.columns[1]._vals)
    for k in range(n - 40, n):
        s0[k] = s1[k] = b"7"
    for j, c in enumerate(cells0):
        s0[n - len(cells0) + j] = c
    if cells1:
        for j, c in enumerate(cells1):
            s1[n - len(cells1) + j] = c
    return Chunk([StrColumn(s0), StrColumn(s1), chk.columns[2], chk.columns[3]])


@pytest.mark.parametrize("jit", [abi.JIT_OFF, abi.JIT_FORCE])
def test_errors_follow_the_last_non_null_row(ctx, jit):
    base = mk_chunk(31, 100_000, vocab())
    big = b"99999999999999999999"
    # an overflowing LAST non-NULL row: ErrOverflow (a NULL after it does not count)
    chk = with_tail(base, [big, None])
    for device in (False, True):
        got = run(ctx, chk, [("s0", None)], R.CTX_SELECT, jit, device=device)
        assert got[4] == abi.ERR_OVERFLOW_BIGINT
        check(got, model(chk, [("s0", None)], R.CTX_SELECT))
    # the same value anywhere else: no error, and the row is true (ParseInt returned MaxInt64)
    chk = with_tail(base, [big, b"7"])
    got = run(ctx, chk, [("s0", None)], R.CTX_SELECT, jit)
    assert got[4] == abi.OK and got[0][-2]
    check(got, model(chk, [("s0", None)], R.CTX_SELECT))
    # a junk last row: ErrTruncatedWrongVal when truncation is an error (DELETE), a warning in a SELECT
    chk = with_tail(base, [b"12abc"])
    assert run(ctx, chk, [("s0", None)], R.CTX_DELETE, jit)[4] == abi.ERR_TRUNCATED_WRONG_VALUE
    check(run(ctx, chk, [("s0", None)], R.CTX_DELETE, jit), model(chk, [("s0", None)], R.CTX_DELETE))
    got = run(ctx, chk, [("s0", None)], R.CTX_SELECT, jit)
    assert got[4] == abi.OK
    check(got, model(chk, [("s0", None)], R.CTX_SELECT))
    # an earlier conjunct's error wins: s1 fails (truncation) before s0 would (overflow) ...
    chk = with_tail(base, [big], [b"x"])
    got = run(ctx, chk, [("s1", None), ("s0", None)], R.CTX_DELETE, jit)
    assert got[4] == abi.ERR_TRUNCATED_WRONG_VALUE
    check(got, model(chk, [("s1", None), ("s0", None)], R.CTX_DELETE))
    # ... and the other way round
    got = run(ctx, chk, [("s0", None), ("s1", None)], R.CTX_DELETE, jit)
    assert got[4] == abi.ERR_OVERFLOW_BIGINT
    check(got, model(chk, [("s0", None), ("s1", None)], R.CTX_DELETE))
    # an evaluation error of an earlier conjunct comes before the string conjunct's toBool error
    ovf = F("gt", F("plus", I2, E.Constant((1 << 63) - 2)), E.Constant(0))
    ce = E.CompiledExpr(ctx, [ovf, S0], jit=jit, str_ctx=R.CTX_DELETE)
    chk2 = with_tail(base, [b"x"])
    try:
        with pytest.raises(_lib.TsqError) as ex:
            ce.VectorizedFilter(chk2)
        assert ex.value.status == abi.ERR_OVERFLOW_BIGINT and "conjunct 0" in ex.value.message
    finally:
        ce.close()
    ce = E.CompiledExpr(ctx, [S0, ovf], jit=jit, str_ctx=R.CTX_DELETE)
    try:
        with pytest.raises(_lib.TsqError) as ex:
            ce.VectorizedFilter(chk2)
        assert ex.value.status == abi.ERR_TRUNCATED_WRONG_VALUE
    finally:
        ce.close()


@pytest.mark.parametrize("jit", [abi.JIT_OFF, abi.JIT_FORCE])
def test_vec_eval_bool_shape_of_the_reference(ctx, jit):
    # expression/bench_test.go:675-694 TestVecEvalBool: 1-5 conjuncts of ETReal / ETString columns, numeric strings in [0, 10)
    rng = np.random.default_rng(3)
    n = 1024
    for it in range(12):
        ncols = int(rng.integers(1, 6))
        kinds = [("real", None) if rng.random() < 0.5 else ("s%d" % int(rng.integers(0, 2)), None) for _ in range(ncols)]
        strs0 = [None if rng.random() < 0.1 else ("%.*f" % (int(rng.integers(0, 3)), rng.random() * 10)).encode() for _ in range(n)]
        strs1 = [None if rng.random() < 0.1 else str(int(rng.integers(0, 10))).encode() for _ in range(n)]
        reals = Column(abi.F64, rng.random(n) * 10, rng.random(n) >= 0.1)
        chk = Chunk([StrColumn(strs0), StrColumn(strs1), Column(abi.I64, np.zeros(n, np.int64)), reals])
        want = model(chk, kinds, R.CTX_SELECT)
        check(run(ctx, chk, kinds, R.CTX_SELECT, jit), want)
        # the row form (EvalBool -> Datum.ToBool) uses the same StrToInt: every row alone gives the same answer
        for i in rng.integers(0, n, 8):
            one = Chunk([StrColumn([strs0[i]]), StrColumn([strs1[i]]), Column(abi.I64, np.zeros(1, np.int64)),
                         Column(abi.F64, reals.data[i:i + 1], reals.notnull[i:i + 1])])
            assert run(ctx, one, kinds, R.CTX_SELECT, jit)[0][0] == want[0][i]


def test_projection_of_a_string_root_still_refused(ctx):
    ce = E.CompiledExpr(ctx, [S0])
    try:
        with pytest.raises(_lib.TsqError) as ex:
            ce.VecEval(mk_chunk(1, 10, BASE))
        assert ex.value.status == abi.ERR_UNSUPPORTED
    finally:
        ce.close()


def test_str_ctx_with_an_unknown_bit_is_invalid(ctx):
    with pytest.raises(_lib.TsqError) as ex:
        E.CompiledExpr(ctx, [S0], str_ctx=16)
    assert ex.value.status == abi.ERR_INVALID


def test_gpu_selection_exec_with_a_string_conjunct(ctx):
    from tinysql_amd import gpu_pipeline as GP
    # a SELECT statement: each batch is its own call, so the vocabulary holds only strings whose conversion raises no error
    ok = [s for s in vocab() if not R.str_to_int(s, R.CTX_SELECT)[1] & (R.ERR_OVF | R.ERR_TRUNC)]
    chk = mk_chunk(41, 200_000, ok)
    conjs = [("int", -2), ("s0", None)]
    want = model(chk, conjs, R.CTX_SELECT)
    dev = GP.DeviceChunk.from_host(ctx, chk)
    try:
        exe = GP.GpuSelectionExec(ctx, GP.DeviceTableScan(ctx, dev, batch_rows=65536), [expr_of(k, a) for k, a in conjs], str_ctx=R.CTX_SELECT)
        got = [r for c in GP.drain_device(exe) for r in c.rows()]
        warn = exe.truncated_warnings, exe.overflow_warnings
    finally:
        dev.free()
    # (per batch the counts restart; they add up over the batches)
    rows = chk.rows()
    assert got == [rows[i] for i in np.nonzero(want[0])[0]]
    assert warn == (want[2], want[3])
