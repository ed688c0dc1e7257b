"""CPU: the yardstick of tests/key_edge.py against the CPU oracle — every edge cell against every edge cell as join keys, for every
ordered pair of key types, and the edge cells of every type as GROUP BY keys — the facts of the two rules the GPU tests rely on,
pinned one by one, and the proof that the comparison helpers report a wrong key rule on this grid."""
import math

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd.chunk import Chunk, Column

from . import helpers as H
from . import key_edge as KE

PAIRS = [(b, p) for b in KE.TYPE_NAMES for p in KE.TYPE_NAMES]


def _side(tp, cs):
    return Chunk([KE.column(tp, cs), Column(abi.I64, np.arange(len(cs), dtype=np.int64))])


def _grid(tp):
    """every edge cell twice (not next to each other) and two NULL keys"""
    cs = KE.cells(tp)
    return cs + [None] + cs[::-1] + [None]


def test_the_grid_holds_what_it_names():
    n = {tp: dict(KE.EDGE[tp]) for tp in KE.TYPE_NAMES}
    assert len(KE.EDGE["i64"]) == 13 and len(KE.EDGE["u64"]) == 8 and len(KE.EDGE["f64"]) == 24 and len(KE.EDGE["f32"]) == 15
    assert n["i64"]["sentinel"] & KE.M64 == KE.SENT == n["u64"]["sentinel"] and H.mix64(n["i64"]["unmix(sentinel)"]) == KE.SENT
    assert n["f64"]["+denorm_min"] == 5e-324 and n["f64"]["+dbl_min"] == 2.2250738585072014e-308 and n["f64"]["+dbl_max"] == 1.7976931348623157e308
    assert n["f64"]["0.1f"] == n["f32"]["0.1f"] != 0.1 and n["f64"]["2^24+1"] == 16777217.0 and n["f32"]["2^24+2"] == 16777218.0
    assert n["f32"]["+flt_max"] == 3.4028234663852886e38 and n["f32"]["+denorm_min"] == 1.401298464324817e-45
    nans = [c for c in KE.cells("f64") if math.isnan(c)]
    assert len(nans) == 6 and len({KE.f64_bits(c) for c in nans}) == 6
    assert sum(math.isnan(c) for c in KE.cells("f32")) == 3
    for tp in KE.TYPE_NAMES:  # the cells survive the way into a column and back, bit for bit
        cs = _grid(tp)
        back = KE.cells_of_column(tp, KE.column(tp, cs))
        assert [None if c is None else KE.key_bits(tp, c) for c in back] == [None if c is None else KE.key_bits(tp, c) for c in cs]


# ---------------------------------------------------------------------------------------------------------------- against the oracle
def _oracle_pairs(orc, tpb, build, tpp, probe):
    cfg = H.join_cfg([KE.TYPES[tpp], abi.I64], [KE.TYPES[tpb], abi.I64], [0], [0], abi.JOIN_INNER, 1)
    out = orc.hash_join(cfg, _side(tpb, build), _side(tpp, probe))
    return [(int(r[1]), int(r[3])) for r in out.rows()]


@pytest.mark.parametrize("tpb,tpp", PAIRS, ids=["%s-%s" % p for p in PAIRS])
def test_oracle_join_returns_exactly_the_pairs_of_the_yardstick(orc, tpb, tpp):
    build, probe = _grid(tpb), _grid(tpp)
    want = KE.join_pairs(tpb, build, tpp, probe)
    slow = [(i, j) for i, p in enumerate(probe) for j, b in enumerate(build) if KE.join_equal(tpp, p, tpb, b)]
    assert want == slow  # (the index of join_pairs and the definition)
    assert KE.pairs_mismatch(want, _oracle_pairs(orc, tpb, build, tpp, probe)) == ""
    if (tpb in KE.INT_TYPES) != (tpp in KE.INT_TYPES):
        assert want == []  # flag 5 against flag 8 / 9
    elif tpb == tpp:
        assert len(want) == 4 * len(KE.EDGE[tpb])  # every cell equals itself and nothing else: 2 x 2 rows


def _agg_rows(orc, tp, cs):
    t = [KE.TYPES[tp], abi.I64]
    aggs = [(abi.AGG_FIRSTROW, 0, t[0]), (abi.AGG_COUNT, -1, abi.I64), (abi.AGG_SUM, 1, abi.I64), (abi.AGG_MIN, 1, abi.I64)]
    return orc.hash_agg(H.agg_cfg(t, [0], aggs), _side(tp, cs), 4, 4).rows()


@pytest.mark.parametrize("tp", KE.TYPE_NAMES)
def test_oracle_aggregate_returns_exactly_the_groups_of_the_yardstick(orc, tp):
    cs = _grid(tp) + KE.cells(tp)[:3]
    rows = _agg_rows(orc, tp, cs)
    assert KE.agg_mismatch(tp, cs, list(range(len(cs))), rows) == ""
    assert len(rows) == len(KE.groups_of(tp, cs))


# ---------------------------------------------------------------------------------------------------------------- pinned facts
def test_pinned_facts_of_the_two_rules(orc):
    f = dict(KE.EDGE["f64"])
    g = dict(KE.EDGE["f32"])
    # -0.0 / +0.0: different join keys, one group
    assert not KE.join_equal("f64", f["-0"], "f64", f["+0"]) and KE.group_image("f64", f["-0"]) == KE.group_image("f64", f["+0"]) == 1 << 63
    assert not KE.join_equal("f32", g["-0"], "f64", f["+0"]) and KE.join_equal("f32", g["-0"], "f64", f["-0"])
    # two NaN payloads differ in both rules; equal bits are equal in both
    assert not KE.join_equal("f64", f["nan"], "f64", f["nan_p1"]) and KE.group_image("f64", f["nan"]) != KE.group_image("f64", f["nan_p1"])
    assert KE.join_equal("f64", f["nan"], "f64", f["nan"]) and KE.join_equal("f32", g["nan"], "f64", f["nan"])
    assert not KE.join_equal("f32", g["nan_p1"], "f64", f["nan_p1"])  # (the float32 payload bit 0 is bit 29 of the double)
    # +NaN shares its group with the denormal 0x0007ffffffffffff, and with nothing else on the grid; it is no join key of it
    assert KE.group_image("f64", f["nan"]) == KE.group_image("f64", f["denorm_7ffff"]) == 0x8007FFFFFFFFFFFF
    assert not KE.join_equal("f64", f["nan"], "f64", f["denorm_7ffff"])
    # ... the all-ones NaN with the sign bit clear shares the group of the zeros; NaNs with the sign bit set are alone
    assert KE.group_image("f64", f["nan_pos_ones"]) == 1 << 63
    assert KE.group_image("f64", f["-nan"]) == 0x0007FFFFFFFFFFFF and KE.group_image("f64", f["nan_neg_ones"]) == 0
    groups = KE.groups_of("f64", KE.cells("f64"))
    shared = sorted(sorted(KE.EDGE["f64"][i][0] for i in rows) for rows in groups.values() if len(rows) > 1)
    assert shared == [["+0", "-0", "nan_pos_ones"], ["denorm_7ffff", "nan"]]
    assert sorted(len(r) for r in KE.groups_of("f32", KE.cells("f32")).values()) == [1] * 13 + [2]  # float32: only the zeros meet
    # 0.1f equals neither 0.1 ...
    assert not KE.join_equal("f32", g["0.1f"], "f64", f["0.1"]) and KE.join_equal("f32", g["0.1f"], "f64", f["0.1f"])
    assert KE.group_image("f32", g["0.1f"]) != KE.group_image("f64", f["0.1"])
    # ... and 2^63 as U64 never equals I64_MIN (same bytes, flag 9 against flag 8); as group keys the 64 bits decide
    assert KE.join_flag_word("u64", 1 << 63) == (9, 1 << 63) and KE.join_flag_word("i64", KE.I64_MIN) == (8, 1 << 63)
    assert not KE.join_equal("u64", 1 << 63, "i64", KE.I64_MIN) and KE.join_equal("u64", (1 << 63) - 1, "i64", KE.I64_MAX)
    assert not KE.join_equal("u64", KE.U64_MAX, "i64", -1) and KE.join_equal("u64", KE.U64_MAX, "u64", KE.U64_MAX)
    assert KE.group_image("u64", 1 << 63) == KE.group_image("i64", KE.I64_MIN)
    # NULL: equals nothing, one group
    assert not KE.join_equal("i64", None, "i64", None) and list(KE.groups_of("i64", [None, 1, None]).values()) == [[0, 2], [1]]
    # the oracle says the same about each of these
    assert _oracle_pairs(orc, "f64", [f["-0"], f["nan"], f["denorm_7ffff"], f["0.1"]], "f64", [f["+0"], f["nan_p1"], f["nan"], f["nan"]]) == [(2, 1), (3, 1)]
    assert _oracle_pairs(orc, "f64", [f["0.1"], f["0.1f"]], "f32", [g["0.1f"]]) == [(0, 1)]
    assert _oracle_pairs(orc, "i64", [KE.I64_MIN, -1, KE.I64_MAX], "u64", [1 << 63, KE.U64_MAX, (1 << 63) - 1]) == [(2, 2)]
    rows = _agg_rows(orc, "f64", [f["nan"], f["denorm_7ffff"], f["-0"], f["+0"], f["nan_pos_ones"], f["nan_p1"]])
    assert sorted((int(r[1]), int(r[2])) for r in rows) == [(1, 5), (2, 1), (3, 9)]
    keys = {int(r[1]): KE.f64_bits(r[0]) for r in rows}  # a row's own cell (func_first_row.go:67-81), never a decoded image
    assert keys[2] in (0x7FF8000000000000, 0x0007FFFFFFFFFFFF) and keys[3] in (0, 1 << 63, 0x7FFFFFFFFFFFFFFF) and keys[1] == 0x7FF8000000000001


# ---------------------------------------------------------------------------------------------------------------- the tests bite
def _float_by_value(tpa, a, tpb, b):
    """WRONG on purpose: reals compared as numbers (`==`), the way a kernel that loads doubles would"""
    if a is None or b is None:
        return False
    if tpa in KE.REAL_TYPES and tpb in KE.REAL_TYPES:
        return a == b
    return KE.join_equal(tpa, a, tpb, b)


def _unsigned_flag_ignored(tpa, a, tpb, b):
    """WRONG on purpose: integers compared by their 8 bytes alone"""
    if a is None or b is None:
        return False
    if tpa in KE.INT_TYPES and tpb in KE.INT_TYPES:
        return KE.key_bits(tpa, a) == KE.key_bits(tpb, b)
    return KE.join_equal(tpa, a, tpb, b)


def _image_raw_bits(tp, cell):
    """WRONG on purpose: reals grouped by their raw bits (-0.0 and +0.0 apart, no NaN with a denormal)"""
    return None if cell is None else KE.key_bits(tp, cell)


def test_the_comparison_reports_a_wrong_key_rule_on_the_grid():
    for tpb, tpp in (("f64", "f64"), ("f32", "f64"), ("f64", "f32"), ("f32", "f32")):
        build, probe = _grid(tpb), _grid(tpp)
        wrong = KE.join_pairs(tpb, build, tpp, probe, equal=_float_by_value)
        msg = KE.pairs_mismatch(KE.join_pairs(tpb, build, tpp, probe), wrong)
        assert "pairs missing" in msg and "[]" not in msg.split("pairs too many")[0], (tpb, tpp, msg)  # NaN == NaN is false: pairs are missing
        assert "pairs too many: []" not in msg, (tpb, tpp, msg)                                        # -0.0 == +0.0: pairs too many
    for tpb, tpp in (("i64", "u64"), ("u64", "i64")):
        build, probe = _grid(tpb), _grid(tpp)
        wrong = KE.join_pairs(tpb, build, tpp, probe, equal=_unsigned_flag_ignored)
        msg = KE.pairs_mismatch(KE.join_pairs(tpb, build, tpp, probe), wrong)
        assert "pairs missing: []" in msg and "pairs too many: []" not in msg, (tpb, tpp, msg)  # 2^63 meets I64_MIN, the sentinels meet
    for tpb, tpp in (("i64", "i64"), ("u64", "u64")):  # (where the flag cannot differ the wrong rule is right: nothing to report)
        build, probe = _grid(tpb), _grid(tpp)
        assert KE.pairs_mismatch(KE.join_pairs(tpb, build, tpp, probe), KE.join_pairs(tpb, build, tpp, probe, equal=_unsigned_flag_ignored)) == ""
    for tp in KE.REAL_TYPES:
        cs = _grid(tp)
        args = list(range(len(cs)))
        wrong_groups = KE.groups_of(tp, cs, image=_image_raw_bits)
        assert KE.groups_mismatch(KE.groups_of(tp, cs), wrong_groups.values()) != ""
        wrong_rows = [(cs[r[0]], len(r), sum(args[i] for i in r), min(args[i] for i in r)) for r in wrong_groups.values()]
        assert KE.agg_mismatch(tp, cs, args, wrong_rows) != ""
    # a decoded image in place of a member cell: the group of +NaN alone comes out as the denormal no row holds
    f = dict(KE.EDGE["f64"])
    assert "no cell of the group" in KE.agg_mismatch("f64", [f["nan"], f["nan"]], [0, 1], [(f["denorm_7ffff"], 2, 1, 0)])
    assert KE.agg_mismatch("f64", [f["nan"], f["denorm_7ffff"]], [0, 1], [(f["denorm_7ffff"], 2, 1, 0)]) == ""
    assert KE.agg_mismatch("f64", [f["nan"], f["denorm_7ffff"]], [0, 1], [(f["nan"], 2, 1, 0)]) == ""
