"""The shared edge-value grid of the expression tests (tests/test_expr_edge_cpu.py, tests/test_expr_edge_gpu.py,
tests/test_join_conds_edge_gpu.py) and its classification by the oracle.

Columns are those of test_hostsim_vs_oracle.cols_for: [I64, I64, U64, U64, F64, F64, F32].  Every type has 21 values, the last one
NULL; row (a, b) is [iv[a], iv[b], uv[a], uv[b], fv[a], fv[b], f32[(a + b) % 21]], 441 rows.  The values sit on the boundaries of the
overflow checks of tsq_eval_row (2^31, 2^32, sqrt(2^63), 2^62, 2^63, 2^64), of the reals (+-0.0, denormals, DBL_MAX, sqrt(DBL_MAX),
DBL_MAX / 2, 2^53 + 1, +inf), of toBool's |f| < 0.5 and of the f32 -> f64 widening (denormals, FLT_MIN, FLT_MAX, 2^24).

An error aborts a whole chunk, so the oracle is asked row by row: classify() gives, per expression (or CNF list), the rows that
evaluate and the rows that raise with their status.  The oracle is the reference, quirks included (builtin_arithmetic_vec.go:454
compares lh with lh, MinInt64 * -1 is not reported, the no_unsigned_subtraction forms have their own rules): no range rule here."""
import numpy as np

from tinysql_amd import _abi as abi
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column

from .test_hostsim_vs_oracle import all_exprs

I, U, R = abi.I64, abi.U64, abi.F64
TYPES = [I, I, U, U, R, R, abi.F32]
I64MAX, I64MIN, U64MAX = (1 << 63) - 1, -(1 << 63), (1 << 64) - 1

IV = [0, 1, -1, I64MAX, I64MIN, I64MAX - 1, I64MIN + 1, 2, -2, 1 << 62, -(1 << 62), 3037000499, 3037000500, -3037000500,
      1 << 32, -(1 << 32), 1 << 31, -(1 << 31), (1 << 31) - 1, 4294967295, None]
UV = [0, 1, U64MAX, U64MAX - 1, 1 << 63, (1 << 63) - 1, (1 << 63) + 1, 2, 3, 1 << 62, 5, 4294967295, 4294967296, 4294967297,
      3037000500, 6074001000, 1 << 32, 1 << 31, (1 << 33) - 1, U64MAX // 3, None]
FV = [0.0, -0.0, 1.0, -1.0, 1.7976931348623157e308, -1.7976931348623157e308, 5e-324, -5e-324, 2.2250738585072014e-308, 0.4, 0.5,
      0.49999999999999994, -0.5, 1.3407807929942597e154, 1.3407807929942596e154, 8.98846567431158e307, 2.0,
      1e-300, 9007199254740993.0, float("inf"), None]
F32V = [0.0, -0.0, 1.0, 1e-45, -1e-45, 1.1754942e-38, 1.17549435e-38, 3.4028235e38, -3.4028235e38, 16777216.0,
        0.5, 0.49999997, 0.1, 1e-30, 1e30, 2.0, -1.0, 3.0, 7.0, 100.0, None]
NV = 21
assert len(IV) == len(UV) == len(FV) == len(F32V) == NV
NROWS = NV * NV
BIG = 4133  # 16 whole workgroups of 256 rows and a ragged tail of 37; >= 4096: jit_expr writes bitmap words itself (counters[2])


def _column(tp, vals, dtype):
    nn = np.array([v is not None for v in vals], bool)
    if dtype in (np.int64, np.uint64):
        data = np.array([0 if v is None else int(v) for v in vals], dtype=dtype)
    else:
        with np.errstate(over="ignore", under="ignore"):
            data = np.array([0.0 if v is None else v for v in vals], dtype=np.float64).astype(dtype)
    return Column(tp, data, nn)


_grid = None


def grid():
    """the 441-row chunk (one instance: nobody writes to it)"""
    global _grid
    if _grid is None:
        a, b = np.divmod(np.arange(NROWS), NV)
        pick = lambda vals, ix: [vals[i] for i in ix]  # noqa: E731
        _grid = Chunk([_column(I, pick(IV, a), np.int64), _column(I, pick(IV, b), np.int64),
                       _column(U, pick(UV, a), np.uint64), _column(U, pick(UV, b), np.uint64),
                       _column(R, pick(FV, a), np.float64), _column(R, pick(FV, b), np.float64),
                       _column(abi.F32, pick(F32V, (a + b) % NV), np.float32)])
        f32 = _grid.columns[6].data
        assert f32[3] != 0 and abs(f32[3]) < 1.2e-38 and np.isfinite(f32).all()  # the f32 denormals are denormals here
    return _grid


def take(chk, idx):
    """the rows idx (any order, repeats allowed) of a fixed-width chunk"""
    idx = np.asarray(idx, np.int64)
    return Chunk([Column(c.tp, c.data[idx], None if c.notnull is None else c.notnull[idx]) for c in chk.columns])


_rows = None


def single_rows():
    """the grid as 441 one-row chunks"""
    global _rows
    if _rows is None:
        g = grid()
        _rows = [g.slice(r, r + 1) for r in range(NROWS)]
    return _rows


class Classified:
    """ok: indices of the rows that evaluate; err: [(row, status)]; per_row[r]: the oracle's answer for row r alone —
    ("ok", data word, notnull, warnings) for an expression, ("ok", selected, isnull, warnings) for a list, or ("err", status)"""

    def __init__(self, per_row):
        self.per_row = per_row
        self.ok = np.array([r for r, p in enumerate(per_row) if p[0] == "ok"], np.int64)
        self.err = [(r, p[1]) for r, p in enumerate(per_row) if p[0] == "err"]

    def one_per_status(self):
        """{status: first grid row that raises it}"""
        out = {}
        for r, s in self.err:
            out.setdefault(s, r)
        return out


_cache = {}


def classify(orc, e):
    """e: one expression (orc.expr_eval per row) or a list of conjuncts (orc.filter_eval per row)"""
    is_list = isinstance(e, (list, tuple))
    progs = E.compile_list(list(e)) if is_list else E.compile_expr(e)
    key = (is_list, len(e) if is_list else 1, bytes(progs))
    if key in _cache:
        return _cache[key]
    per_row = []
    for one in single_rows():
        try:
            if is_list:
                s, z, w = orc.filter_eval(progs, len(e), one)
                per_row.append(("ok", bool(s[0]), bool(z[0]), w))
            else:
                col, w = orc.expr_eval(progs, one)
                nn = col.notnull is None or bool(col.notnull[0])
                per_row.append(("ok", int(col.data.view(np.uint64)[0]), nn, w))
        except orc.OracleError as ex:
            per_row.append(("err", ex.status))
    _cache[key] = Classified(per_row)
    return _cache[key]


# ---------------------------------------------------------------- the expressions, by family
def family(e):
    if isinstance(e, E.ScalarFunction) and e.name in ("plus", "minus", "mul") and e.eval_type == E.ETInt:
        return "minus_signed" if e.force_signed else e.name
    if e.eval_type == E.ETReal:
        return "real"
    if isinstance(e, E.ScalarFunction) and e.name in ("lt", "le", "gt", "ge", "eq", "ne"):
        return "compare"
    return "rest"


FAMILIES = ["plus", "minus", "mul", "minus_signed", "real", "compare", "rest"]


def exprs_of(fam):
    return [(i, e) for i, e in enumerate(all_exprs()) if family(e) == fam]


def _parts(names, items_of, size):
    """{id: items}: the items of every name in parts of at most `size` (a hiprtc compile per item: a GPU test stays at a few seconds)"""
    out = {}
    for name in names:
        items = items_of(name)
        n = (len(items) + size - 1) // size
        for k in range(n):
            out[name if n == 1 else "%s_%d" % (name, k)] = items[k * size:(k + 1) * size]
    return out


EXPR_PARTS = _parts(FAMILIES, exprs_of, 10)


def is_arithmetic(e):
    return isinstance(e, E.ScalarFunction) and e.name in ("plus", "minus", "mul", "div", "unaryminus")


C = {i: E.Column(i, t) for i, t in enumerate(TYPES)}
F, K = E.ScalarFunction, E.Constant
B0 = F("gt", C[0], K(0))
ISNULL_OR = F("or", F("isnull", C[0]), F("gt", C[1], K(0)))
LIST_KINDS = ["single", "b0_first", "b0_last", "isnull_or_real"]


def filter_lists(kind):
    """[(index in all_exprs(), conjunct list)]: every arithmetic expression as a single conjunct, behind and in front of
    b0 = gt(c0, 0) (alive / NULL bookkeeping, the conjunct index of the error word), the real ones behind an Int conjunct
    that can be NULL"""
    out = []
    for i, e in enumerate(all_exprs()):
        if not is_arithmetic(e):
            continue
        if kind == "single":
            out.append((i, [e]))
        elif kind == "b0_first":
            out.append((i, [B0, e]))
        elif kind == "b0_last":
            out.append((i, [e, B0]))
        elif e.eval_type == E.ETReal:
            out.append((i, [ISNULL_OR, e]))
    return out


LIST_PARTS = _parts(LIST_KINDS, filter_lists, 9)


# ---------------------------------------------------------------- trees with several fallible nodes (first-error order)
def order_trees():
    """[(name, tree, [fallible sub-expressions in the evaluation order of the node-at-a-time evaluator: children left to right,
    then the node])].  A row's failing node is the first of them that raises on the row."""
    p01, m23 = F("plus", C[0], C[1]), F("minus", C[2], C[3])
    t1 = F("mul", p01, m23)
    im = F("mul", C[0], F("plus", F("in", C[0], K(I64MAX)), K(1)))  # c0 * (1 or 2)
    p23 = F("plus", C[2], C[3])
    t2 = F("mul", im, F("isnull", p23))
    pr, mi, mu = F("plus", C[4], C[5]), F("mul", C[0], C[1]), F("minus", C[2], C[3])
    t3 = F("if", F("gt", pr, K(0.0)), mi, mu)
    fs = F("minus", C[0], C[3], no_unsigned_subtraction=True)  # raises BIGINT or BIGINT UNSIGNED at ONE node
    m01 = F("mul", C[0], C[1])
    t4 = F("plus", fs, m01)
    return [("mul_plus_minus", t1, [p01, m23, t1]), ("mul_mul_in_isnull_plus", t2, [im, p23]),
            ("if_real_int_uint", t3, [pr, mi, mu]), ("plus_forced_minus_mul", t4, [fs, m01, t4])]


def failing_nodes(orc, tree, subs):
    """{grid row: (index into subs, status)} for the rows on which the tree raises"""
    whole = classify(orc, tree)
    parts = [classify(orc, s) for s in subs]
    out = {}
    for r, st in whole.err:
        for k, p in enumerate(parts):
            if p.per_row[r][0] == "err":
                assert p.per_row[r][1] == st, "the tree's status on one row is that of its first failing node"
                out[r] = (k, st)
                break
        else:
            raise AssertionError("row %d raises in the tree but in none of its fallible nodes" % r)
    return out


def tiled(ok, n):
    """n grid-row indices: the error-free rows over and over"""
    return np.resize(np.asarray(ok, np.int64), n)


INSERT_AT = [0, 1, 2, 3, 63, 64, 255, 256, -1]  # the four row slots of a JIT lane, both sides of a wave and of a workgroup edge, last
SMALL = 300  # rows of the chunk an error row is inserted into (>= 257, so that every position exists)


def with_row(base_idx, row, k):
    """base_idx with grid row `row` inserted at the k-th position of INSERT_AT's cycle"""
    pos = INSERT_AT[k % len(INSERT_AT)]
    pos = len(base_idx) if pos < 0 else min(pos, len(base_idx))
    return np.insert(base_idx, pos, row), pos
