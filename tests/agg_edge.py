"""The yardstick of the aggregate functions at their edge values: named groups of argument cells per argument type, and a plain, exact
statement of which results are legitimate for COUNT / SUM / AVG / MIN / MAX over such a group.  No GPU and no oracle in here: Python
ints, fractions.Fraction, bit patterns through struct / numpy.

  sum4Float64 / sum4Int64       executor/aggfuncs/func_sum.go:62-90, 117-154   (the first value is ASSIGNED, later ones are added)
  avgOriginal4* / baseAvg*      executor/aggfuncs/func_avg.go:47-55, 154-183   (integer AVG: Go's `/`, truncated toward zero)
  maxMin4Float64 / Int / Uint   executor/aggfuncs/func_max_min.go:81-117       (`v > cur` / `v < cur`, update and merge)

A cell is None (NULL), an int (I64 / U64) or a float (F64; an F32 cell holds the widened value, exactly representable in 32 bits).

Verdicts (what expected() returns):
  ("null",)                       the result cell is NULL
  ("int", v)                      an exact integer
  ("err", status)                 the statement fails with this status
  ("nan",)                        any NaN
  ("inf", x)                      exactly the infinity x
  ("near", v, t, zneg)            |got - v| <= t; zneg is None unless the exact sum is zero: then a zero result has its sign bit set
                                  iff zneg, which is true iff every non-NULL cell is -0.0 (func_sum.go:72-77 assigns the first value)
  ("near_or_inf", v, t, signs, zneg)  as "near" (v is None where the exact sum rounds to an infinity), or an infinity whose sign is in
                                  `signs` (NaN as well where both signs are: two partial sums of opposite infinities may meet)
  ("one_of", bits)                the bit pattern of the result, in the argument's own width, is a member of the frozenset `bits`
"""
import math
import struct
from fractions import Fraction

import numpy as np

from tinysql_amd import _abi as abi

I64MIN, I64MAX, U64MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
DBL_MAX, DBL_MIN, DBL_DENORM = 1.7976931348623157e308, 2.2250738585072014e-308, 5e-324
FLT_MAX, FLT_MIN, FLT_DENORM = 3.4028234663852886e38, 1.1754943508222875e-38, 1.401298464324817e-45
INF, NAN = math.inf, math.nan
# the least magnitude that rounds to an infinity: DBL_MAX + half an ulp
ROUNDS_TO_INF = Fraction(2) ** 1024 - Fraction(2) ** 970

FUNCS = ("count", "sum", "avg", "min", "max")
FUNC_CODE = {"count": abi.AGG_COUNT, "sum": abi.AGG_SUM, "avg": abi.AGG_AVG, "min": abi.AGG_MIN, "max": abi.AGG_MAX}
TYPES = {"i64": abi.I64, "u64": abi.U64, "f64": abi.F64, "f32": abi.F32}


def f64_from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def f32_from_bits(b):
    """the float32 with these bits, widened (exact; a NaN keeps its sign and the top of its payload)"""
    return float(np.array([b], dtype=np.uint32).view(np.float32)[0])


def bits_of(v, tp):
    """bit pattern of a real cell in the width of type `tp` ("f64": 64 bits, "f32": 32 bits)"""
    if tp == "f32":
        return int(np.array([v], dtype=np.float64).astype(np.float32).view(np.uint32)[0])
    return struct.unpack("<Q", struct.pack("<d", v))[0]


# NaNs whose order images (tsq_agg.hip ord_image) are the identity words of MAX and MIN: sign bit set + all-ones mantissa -> 0,
# sign bit clear + all-ones mantissa -> ~0
NAN_NEG_ONES, NAN_POS_ONES, NAN_NEG = f64_from_bits(0xFFFFFFFFFFFFFFFF), f64_from_bits(0x7FFFFFFFFFFFFFFF), f64_from_bits(0xFFF8000000000000)
NAN32_NEG_ONES, NAN32_POS_ONES, NAN32_NEG = f32_from_bits(0xFFFFFFFF), f32_from_bits(0x7FFFFFFF), f32_from_bits(0xFFC00000)

# name -> cells.  `transient`: the row orders ("fwd", "rev") in which a RUNNING int64 sum leaves BIGINT although the final sum fits
# (tests/test_agg_gpu.py test_sum_int64_running_overflow_divergence_is_pinned: an error in the reference with one worker, a value here).
_INT_GROUPS = [
    ("min_alone", [I64MIN]),
    ("max_alone", [I64MAX]),
    ("min_and_max", [I64MIN, I64MAX]),
    ("transient_max_1_m2", [I64MAX, 1, -2]),
    ("final_over", [I64MAX, 1]),
    ("final_under", [I64MIN, -1]),
    ("300max_300min", [I64MAX] * 300 + [I64MIN] * 300),
    ("pm_2_31_m1", [(1 << 31) - 1, -((1 << 31) - 1), (1 << 31) - 1]),
    ("pm_2_31", [1 << 31, -(1 << 31), -(1 << 31)]),
    ("pm_2_32_m1", [(1 << 32) - 1, -((1 << 32) - 1), (1 << 32) - 1, (1 << 32) - 1]),
    ("pm_2_32", [1 << 32, -(1 << 32), -(1 << 32), 1 << 32, 1 << 32]),
    ("2_16_words", [(1 << 16) - 1, 1 << 16, (1 << 16) - 1, 1 << 16]),
    ("word_carries", [(1 << 32) - 1, 1, (1 << 32) - 1, 1, -(1 << 32), (1 << 31), (1 << 31) - 1]),
    ("minus_ones", [-1] * 9),
    ("avg_m7_0", [-7, 0]),
    ("avg_m1x3_2", [-1, -1, -1, 2]),
    ("avg_7_0", [7, 0]),
    ("zero_alone", [0]),
    ("all_null", [None, None, None]),
    ("nulls_between", [None, 5, None, -9, None]),
    ("nulls_around_min", [None, I64MIN, None]),
]
TRANSIENT = {"transient_max_1_m2": ("fwd",), "300max_300min": ("fwd", "rev")}
_U64_GROUPS = [
    ("zero_alone", [0]),
    ("ones_alone", [U64MAX]),
    ("around_2_63", [(1 << 63) - 1, 1 << 63]),
    ("zero_and_ones", [0, U64MAX]),
    ("all_null", [None, None]),
    ("nulls_between", [None, U64MAX, None, 1 << 63, None]),
]


def _real_groups(big, tiny_norm, denorm, nan_neg, nan_neg_ones, nan_pos_ones):
    return [
        ("neg_zero", [-0.0]),
        ("neg_zero_twice", [-0.0, -0.0]),
        ("neg_then_pos_zero", [-0.0, 0.0]),
        ("pos_then_neg_zero", [0.0, -0.0]),
        ("neg_zero_and_null", [None, -0.0, None]),
        ("pos_inf", [INF]),
        ("neg_inf", [-INF]),
        ("pos_inf_and_one", [INF, 1.0]),
        ("both_infs", [INF, -INF]),
        ("nan_alone", [NAN]),
        ("nan_between", [1.0, NAN, 2.0]),
        ("nan_first", [NAN, 1.0]),
        ("neg_nan_alone", [nan_neg]),
        ("neg_nan_beside", [3.0, nan_neg, -4.0]),
        ("neg_ones_nan_alone", [nan_neg_ones]),
        ("neg_ones_nan_beside", [nan_neg_ones, -2.0, 5.0]),
        ("pos_ones_nan_alone", [nan_pos_ones]),
        ("pos_ones_nan_beside", [7.0, nan_pos_ones, -1.0]),
        ("nan_and_infs", [-INF, NAN, INF]),
        ("denorm_x100", [denorm] * 100),
        ("denorm_beside_min_normal", [denorm, tiny_norm, -denorm * 3]),
        ("one_alone", [1.0]),
        ("all_null", [None, None, None]),
        ("nulls_between", [None, 2.5, None, -0.5, None]),
    ]


_F64_GROUPS = _real_groups(DBL_MAX, DBL_MIN, DBL_DENORM, NAN_NEG, NAN_NEG_ONES, NAN_POS_ONES) + [
    ("cancel_1e16", [1e16, 1.0, -1e16]),
    ("max_max_mmax", [DBL_MAX, DBL_MAX, -DBL_MAX]),
    ("max_max", [DBL_MAX, DBL_MAX]),
    ("mmax_alone", [-DBL_MAX]),
]
_F32_GROUPS = _real_groups(FLT_MAX, FLT_MIN, FLT_DENORM, NAN32_NEG, NAN32_NEG_ONES, NAN32_POS_ONES) + [
    ("cancel_2_25", [float(1 << 25), 1.0, -float(1 << 25)]),
    ("flt_max_x4", [FLT_MAX] * 4),          # the sum is a double: no overflow
    ("flt_max_and_back", [FLT_MAX, FLT_MAX, -FLT_MAX]),
    ("f32_denorms_widen", [FLT_DENORM, FLT_DENORM * 3, -FLT_DENORM * 2, FLT_MIN]),
]
EDGE_GROUPS = {"i64": _INT_GROUPS, "u64": _U64_GROUPS, "f64": _F64_GROUPS, "f32": _F32_GROUPS}
# the least table the issue lists, per type (tests/test_agg_edge_cpu.py asserts it)
MIN_GROUPS = {"i64": 18, "u64": 4, "f64": 22, "f32": 21}
# U64 arguments: COUNT / MIN / MAX only (SUM / AVG over unsigned arguments are out of scope)
FUNCS_OF = {"i64": FUNCS, "u64": ("count", "min", "max"), "f64": FUNCS, "f32": FUNCS}


def go_div(a, b):
    """Go's integer `/`: truncated toward zero"""
    q = abs(a) // abs(b)
    return q if (a < 0) == (b < 0) else -q


def expected(func, tp, cells):
    """the verdict for `func` over the argument cells of one group (type `tp` in "i64" / "u64" / "f64" / "f32")"""
    vals = [c for c in cells if c is not None]
    if func == "count":
        return ("int", len(vals))
    if not vals:
        return ("null",)
    if tp in ("i64", "u64"):
        if func == "min":
            return ("int", min(vals))
        if func == "max":
            return ("int", max(vals))
        assert tp == "i64", "SUM / AVG over U64 arguments are out of scope"
        s = sum(vals)
        if not I64MIN <= s <= I64MAX:  # DESIGN.md "Documented divergences": an error iff the exact FINAL sum leaves BIGINT
            return ("err", abi.ERR_OVERFLOW_BIGINT)
        return ("int", s if func == "sum" else go_div(s, len(vals)))
    nans = [v for v in vals if math.isnan(v)]
    if func in ("min", "max"):
        nums = [v for v in vals if not math.isnan(v)]
        members = {bits_of(v, tp) for v in nans}  # a NaN that arrives first stays: no `v > NaN` is ever true
        if nums:
            ext = min(nums) if func == "min" else max(nums)
            members |= {bits_of(v, tp) for v in nums if v == ext}  # either zero where both tie
        return ("one_of", frozenset(members))
    infs = {v for v in vals if math.isinf(v)}
    if nans or len(infs) == 2:
        return ("nan",)
    if infs:
        return ("inf", infs.pop())
    n = len(vals)
    ex = [Fraction(v) for v in vals]
    S, A = sum(ex), sum(abs(x) for x in ex)
    t = 2 * n * Fraction(2) ** -53 * A  # the re-ordering bound of a sum of n terms
    if func == "avg":
        S, t = S / n, t / n + (A / n) * Fraction(2) ** -52  # tests/test_agg_gpu.py group_tols
    zneg = all(math.copysign(1.0, v) < 0 and v == 0 for v in vals) if S == 0 else None
    value = float(S) if abs(S) < ROUNDS_TO_INF else None
    if A <= Fraction(DBL_MAX):
        return ("near", value, float(t), zneg)
    # some order of the additions may pass through an infinity: the cells of one sign first.  One cell alone never rounds to an
    # infinity; a partial sum of several carries a relative error of at most (n - 1) 2^-53
    slack = 1 + (n - 1) * Fraction(2) ** -53
    signs = set()
    pos, neg = [x for x in ex if x > 0], [-x for x in ex if x < 0]
    if len(pos) >= 2 and sum(pos) * slack >= ROUNDS_TO_INF:
        signs.add(1)
    if len(neg) >= 2 and sum(neg) * slack >= ROUNDS_TO_INF:
        signs.add(-1)
    return ("near_or_inf", value, float(t), frozenset(signs), zneg)


def satisfies(verdict, got, tp, zero_sign=True):
    """does the result cell `got` (None, int or float, as Chunk.rows() gives it) satisfy the verdict?  Returns "" or what is wrong.
    zero_sign=False: a zero sum is compared by value alone (the CPU oracle, whose real sums start at +0.0)."""
    kind = verdict[0]
    if kind == "err":
        return "the statement should have failed with status %d" % verdict[1]
    if kind == "null":
        return "" if got is None else "want NULL, got %r" % (got,)
    if got is None:
        return "got NULL, want %r" % (verdict,)
    if kind == "int":
        return "" if not isinstance(got, float) and int(got) == verdict[1] else "want %d, got %r" % (verdict[1], got)
    if kind == "nan":
        return "" if math.isnan(got) else "want NaN, got %r" % got
    if kind == "inf":
        return "" if got == verdict[1] else "want %r, got %r" % (verdict[1], got)
    if kind == "one_of":
        b = bits_of(got, tp)
        return "" if b in verdict[1] else "bits %x are none of %s" % (b, sorted("%x" % m for m in verdict[1]))
    value, t, zneg = verdict[1], verdict[2], verdict[-1]
    if kind == "near_or_inf":
        signs = verdict[3]
        if math.isinf(got):
            return "" if (1 if got > 0 else -1) in signs else "infinity of a sign no order of additions reaches: %r" % got
        if math.isnan(got):
            return "" if len(signs) == 2 else "NaN, but only one infinity is reachable"
    if value is None or math.isnan(got) or math.isinf(got):
        return "want about %r, got %r" % (value, got)
    if abs(Fraction(got) - Fraction(value)) > Fraction(t):
        return "want %r within %r, got %r" % (value, t, got)
    if zero_sign and zneg is not None and got == 0 and (math.copysign(1.0, got) < 0) != zneg:
        return "a zero sum of the wrong sign: got %r, every cell is -0.0: %s" % (got, zneg)
    return ""


def verdict_class_counts():
    """{verdict kind: how many (function, type, group) triples carry it}"""
    out = {}
    for tp, groups in EDGE_GROUPS.items():
        for _, cells in groups:
            for func in FUNCS_OF[tp]:
                k = expected(func, tp, cells)[0]
                out[k] = out.get(k, 0) + 1
    return out
