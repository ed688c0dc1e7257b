"""Pins the calculator of tests/agg_edge.py before anyone trusts it on the device: for every (function, argument type, edge group) the CPU
oracle — the C++ restatement of the reference's UpdatePartialResult / MergePartialResult / AppendFinalResult2Chunk — runs the group's
cells in the given and in the reversed row order with one partial and one final worker, and each answer must satisfy the verdict.

Two exceptions, both stated where they are made:
  * the transient integer overflow of tests/test_agg_gpu.py::test_sum_int64_running_overflow_divergence_is_pinned: the oracle adds row by
    row and fails as soon as a running sum leaves BIGINT; the verdict (the project's documented rule) is a value.  Asserted by name, for
    exactly the groups of agg_edge.TRANSIENT and the row orders listed there.
  * a real-valued SUM / AVG of exactly zero is compared by value, not by sign bit.  The sign of a zero sum in the verdict comes from
    the REFERENCE (func_sum.go:72-77 assigns the first value of a group, so SUM({-0.0}) is -0.0); the oracle merges its one partial
    result into a final one that starts at +0.0 and so answers +0.0 for an all -0.0 group in either order.  The oracle's answer is no
    evidence about the sign."""
import math

import pytest

from tinysql_amd import _abi as abi

from . import agg_edge as AE
from . import helpers as H

CASES = [(tp, name) for tp in AE.EDGE_GROUPS for name, _ in AE.EDGE_GROUPS[tp]]


def _oracle(orc, func, tp, cells):
    """the oracle's result cell of a scalar aggregate over `cells`, or ("err", status)"""
    from oracle.binding import OracleError
    t = AE.TYPES[tp]
    aggs = [(AE.FUNC_CODE[func], 0, t)]
    chk = H.chunk_from_rows([[c] for c in cells], [t])
    try:
        out = orc.hash_agg(H.agg_cfg([t], [], aggs), chk, 1, 1)
    except OracleError as e:
        return ("err", e.status)
    rows = out.rows()
    assert len(rows) == 1
    return rows[0][0]


@pytest.mark.parametrize("tp,name", CASES, ids=["%s-%s" % c for c in CASES])
def test_oracle_satisfies_the_verdicts_in_both_row_orders(orc, tp, name):
    cells = dict(AE.EDGE_GROUPS[tp])[name]
    checked = 0
    for func in AE.FUNCS_OF[tp]:
        verdict = AE.expected(func, tp, cells)
        for order, seq in (("fwd", cells), ("rev", cells[::-1])):
            got = _oracle(orc, func, tp, seq)
            if tp == "i64" and func in ("sum", "avg") and order in AE.TRANSIENT.get(name, ()):
                # the pinned divergence: a running sum outside BIGINT is an error there, the exact final sum a value here
                assert verdict[0] == "int" and got == ("err", abi.ERR_OVERFLOW_BIGINT), (func, order, got, verdict)
            elif verdict[0] == "err":
                assert got == verdict, (func, order, got, verdict)
            else:
                assert not isinstance(got, tuple), (func, order, got, verdict)
                # zero_sign=False: the oracle's real sums start at +0.0 (see the module's docstring)
                wrong = AE.satisfies(verdict, got, tp, zero_sign=False)
                assert wrong == "", (func, order, wrong)
            checked += 1
    assert checked == 2 * len(AE.FUNCS_OF[tp])


def test_transient_groups_are_exactly_the_designed_ones(orc):
    """no other integer group fails in the oracle without its verdict saying so"""
    seen = {}
    for name, cells in AE.EDGE_GROUPS["i64"]:
        if AE.expected("sum", "i64", cells)[0] == "err":
            continue
        orders = tuple(o for o, seq in (("fwd", cells), ("rev", cells[::-1])) if isinstance(_oracle(orc, "sum", "i64", seq), tuple))
        if orders:
            seen[name] = orders
    assert seen == AE.TRANSIENT


@pytest.mark.parametrize("tp", ["f64", "f32"])
def test_one_of_sets_are_as_narrow_as_the_row_order_allows(orc, tp):
    """the two row orders give two DIFFERENT members of a `one_of` set on at least one group with a NaN and on one with both zeros:
    a narrower set would refuse a legitimate answer of the reference's `v > cur` protocol"""
    nan_groups, zero_groups = set(), set()
    for name, cells in AE.EDGE_GROUPS[tp]:
        for func in ("min", "max"):
            verdict = AE.expected(func, tp, cells)
            if verdict[0] != "one_of":
                continue
            a, b = (AE.bits_of(_oracle(orc, func, tp, seq), tp) for seq in (cells, cells[::-1]))
            assert a in verdict[1] and b in verdict[1]
            if a != b:
                vals = [c for c in cells if c is not None]
                (nan_groups if any(math.isnan(v) for v in vals) else zero_groups).add(name)
    assert nan_groups and zero_groups, (nan_groups, zero_groups)
    assert zero_groups <= {"neg_then_pos_zero", "pos_then_neg_zero"}


def test_table_size_and_designed_groups():
    for tp, least in AE.MIN_GROUPS.items():
        names = [n for n, _ in AE.EDGE_GROUPS[tp]]
        assert len(names) >= least and len(set(names)) == len(names), tp
    ints = dict(AE.EDGE_GROUPS["i64"])
    assert ints["min_alone"] == [AE.I64MIN] and ints["max_alone"] == [AE.I64MAX] and ints["final_over"] == [AE.I64MAX, 1]
    assert ints["300max_300min"] == [AE.I64MAX] * 300 + [AE.I64MIN] * 300 and set(ints["all_null"]) == {None}
    flat = {abs(c) for cells in ints.values() for c in cells if c is not None}
    assert {(1 << 31) - 1, 1 << 31, (1 << 32) - 1, 1 << 32, (1 << 16) - 1, 1 << 16} <= flat
    assert dict(AE.EDGE_GROUPS["u64"])["zero_and_ones"] == [0, AE.U64MAX]
    for tp in ("f64", "f32"):
        g = dict(AE.EDGE_GROUPS[tp])
        # the NaNs whose order images are the identity words of MAX (0) and MIN (~0)
        assert AE.bits_of(g["neg_ones_nan_alone"][0], tp) == (AE.U64MAX if tp == "f64" else 0xFFFFFFFF)
        assert AE.bits_of(g["pos_ones_nan_alone"][0], tp) == (AE.U64MAX >> 1 if tp == "f64" else 0x7FFFFFFF)
        assert math.copysign(1.0, g["neg_zero"][0]) < 0 and len(g["denorm_x100"]) == 100
        for cells in g.values():  # every F32 cell is a float32 value, widened
            assert all(c is None or math.isnan(c) or tp == "f64" or AE.f32_from_bits(AE.bits_of(c, "f32")) == c for c in cells)
    assert dict(AE.EDGE_GROUPS["f64"])["max_max"] == [AE.DBL_MAX] * 2 and dict(AE.EDGE_GROUPS["f32"])["flt_max_x4"] == [AE.FLT_MAX] * 4


def test_verdicts_of_the_calculator_itself():
    """hand-checked verdicts: the calculator is plain enough to be read, these keep it from drifting"""
    E = AE.expected
    assert E("sum", "i64", [AE.I64MAX, 1, -2]) == ("int", AE.I64MAX - 1)
    assert E("sum", "i64", [AE.I64MAX, 1]) == E("avg", "i64", [AE.I64MIN, -1]) == ("err", abi.ERR_OVERFLOW_BIGINT)
    assert E("avg", "i64", [-7, 0]) == ("int", -3) and E("avg", "i64", [-1, -1, -1, 2]) == ("int", 0) and E("avg", "i64", [7, 0]) == ("int", 3)
    assert E("sum", "i64", [AE.I64MAX] * 300 + [AE.I64MIN] * 300) == ("int", -300)
    assert E("count", "f64", [None, AE.NAN, None]) == ("int", 1) and E("max", "u64", [0, AE.U64MAX]) == ("int", AE.U64MAX)
    assert E("sum", "f64", [None, None]) == ("null",) and E("count", "f64", [None, None]) == ("int", 0)
    assert E("sum", "f64", [-0.0, -0.0])[3] is True and E("avg", "f64", [-0.0, 0.0])[3] is False and E("sum", "f64", [1.0, -1.0])[3] is False
    assert E("sum", "f64", [AE.INF, -AE.INF]) == ("nan",) and E("avg", "f64", [AE.INF, 1.0]) == ("inf", AE.INF)
    assert E("sum", "f64", [AE.DBL_MAX, AE.DBL_MAX])[0] == "near_or_inf" and E("sum", "f64", [AE.DBL_MAX, AE.DBL_MAX])[1] is None
    assert E("sum", "f64", [AE.DBL_MAX, AE.DBL_MAX, -AE.DBL_MAX])[3] == frozenset({1})
    assert E("sum", "f32", [AE.FLT_MAX] * 4)[:2] == ("near", 4 * AE.FLT_MAX)
    assert E("max", "f64", [-0.0, 0.0]) == ("one_of", frozenset({0, 1 << 63})) and E("min", "f64", [1.0, AE.NAN, 2.0])[1] == frozenset(
        {AE.bits_of(1.0, "f64"), AE.bits_of(AE.NAN, "f64")})
    S = AE.satisfies
    assert S(("near", 0.0, 0.0, True), 0.0, "f64") != "" and S(("near", 0.0, 0.0, True), -0.0, "f64") == "" and S(("near", 0.0, 0.0, True), 0.0, "f64", zero_sign=False) == ""
    assert S(("inf", AE.INF), -AE.INF, "f64") != "" and S(("nan",), 1.0, "f64") != "" and S(("int", 3), 3.0, "i64") != "" and S(("null",), 0, "i64") != ""
    assert S(("near_or_inf", 1.0, 0.5, frozenset({1}), None), -AE.INF, "f64") != "" and S(("near_or_inf", 1.0, 0.5, frozenset({1}), None), AE.INF, "f64") == ""
    assert S(("near", 1.0, 0.25, None), 1.5, "f64") != "" and S(("one_of", frozenset({0})), -0.0, "f64") != ""
