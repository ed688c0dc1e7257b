"""GPU: string-valued join OtherConditions and outer filters (toBool's ETString arm, ABI 8).  Expected rows come from the unchanged
oracle running the same join with an Int condition over a precomputed column StrToInt(s) != 0 (NULL where s is NULL: an Int NULL
and a string NULL both leave the row unselected); the warning counts from tests/strtoint_ref.py over the rows / key-matching pairs
the condition is evaluated on.  A join fails with the conversion error iff ANY evaluated row or pair raised one."""
import numpy as np
import pytest

from tests import gpu_helpers as G
from tests import helpers as H
from tests import strtoint_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column, StrColumn

pytestmark = pytest.mark.gpu

# SELECT semantics: no string here raises an error, several raise truncation warnings
WORDS = [b"0", b"1", b"-3", b" 7 ", b"12abc", b"abc", b"", b"0x5", b"00", b"2.5", b"+4", b"-", b"\xc2\xa09"]
BIG = b"99999999999999999999"  # ErrOverflow in a SELECT


def flag_col(cells):
    v = np.array([0 if c is None else int(R.str_to_int(c, R.CTX_SELECT)[0] != 0) for c in cells], np.int64)
    return Column(abi.I64, v, np.array([c is not None for c in cells]))


def tables(seed, nb=5000, npr=20_000, extra=None):
    rng = np.random.default_rng(seed)
    bt = [None if rng.random() < 0.05 else WORDS[k] for k in rng.integers(0, len(WORDS), nb)]
    ps = [None if rng.random() < 0.05 else WORDS[k] for k in rng.integers(0, len(WORDS), npr)]
    if extra is not None:
        ps[extra[0]] = extra[1]
    build = Chunk([Column(abi.I64, np.arange(nb, dtype=np.int64)), StrColumn(bt), Column(abi.I64, rng.integers(-2, 3, nb)), flag_col(bt)])
    probe = Chunk([Column(abi.I64, rng.integers(-500, nb + 500, npr)), StrColumn(ps), flag_col(ps)])
    return build, probe


# joined row (probe is left): probe k0 s1 f2 | build k3 t4 x5 tf6
PS, PF, BT, BX, BF = E.Column(1, abi.BYTES), E.Column(2, abi.I64), E.Column(4, abi.BYTES), E.Column(5, abi.I64), E.Column(6, abi.I64)
F = E.ScalarFunction
CASES = {
    "probe_string": ([PS], [PF]),
    "if_build_x_probe_s_build_t": ([F("if", F("gt", BX, E.Constant(0)), PS, BT)], [F("if", F("gt", BX, E.Constant(0)), PF, BF)]),
}
ROUTES = {"direct": (abi.RADIX_OFF, abi.RADIX_OFF, abi.ROUTE_DIRECT), "packed": (abi.RADIX_FORCE, abi.RADIX_FORCE, abi.ROUTE_PACKED)}


def run(ctx, cfg, build, probe, route):
    radix, packing, _ = ROUTES[route]
    stats = []
    got = G.run_join(ctx, cfg, build, probe, chunk_rows=1 << 22, pull_rows=1 << 20, stats_out=stats, radix=radix, packing=packing)
    return got, stats[0]


def pair_warnings(orc, build, probe, pick):
    """truncation warnings over the key-matching pairs: pick(row) -> the string the condition converts"""
    plain = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1)
    n = 0
    for r in orc.hash_join(plain, build, probe).rows():
        s = pick(r)
        if s is not None:
            n += R.str_to_int(bytes(s), R.CTX_SELECT)[1] & R.TRUNC_WARN
    return n


def to_bytes(x):
    return None if x is None else (x.encode() if isinstance(x, str) else bytes(x))


# string payload columns keep the direct route (the packed routes carry 8-byte cells); the next tests reach k_outer_filter_flags and
# k_post_conds of the packed route with string CONSTANTS chosen by numeric columns
@pytest.mark.parametrize("name", sorted(CASES))
def test_inner_join_string_other_condition_vs_oracle(ctx, orc, name):
    route = "direct"
    build, probe = tables(7)
    gconds, oconds = CASES[name]
    keep = []
    cfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1, gconds, (), keep)
    ocfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1, oconds, (), keep)
    want = orc.hash_join(ocfg, build, probe)
    got, st = run(ctx, cfg, build, probe, route)
    assert st.probe_route == ROUTES[route][2], (st.probe_route, route)
    assert got.NumRows() == want.NumRows() > 1000 and H.rows_equal_unordered(got, want)
    # COUNT(*) of the same join (the row checksum does not cover var-len columns: the rows themselves are compared above)
    c = G.run_join(ctx, cfg, build, probe, chunk_rows=1 << 22, count_only=True, radix=ROUTES[route][0], packing=ROUTES[route][1])
    assert c == want.NumRows()
    if name == "probe_string":
        pick = lambda r: to_bytes(r[1])  # noqa: E731
    else:
        pick = lambda r: to_bytes(r[1] if (r[5] is not None and r[5] > 0) else r[4])  # noqa: E731
    w = pair_warnings(orc, build, probe, pick)
    assert w > 100 and st.str_truncated_warnings == w, (st.str_truncated_warnings, w)
    assert st.str_overflow_warnings == 0


def test_left_outer_join_string_outer_filter_vs_oracle(ctx, orc):
    route = "direct"
    build, probe = tables(8)
    keep = []
    cfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1, (), [PS], keep)
    ocfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1, (), [PF], keep)
    want = orc.hash_join(ocfg, build, probe)
    got, st = run(ctx, cfg, build, probe, route)
    assert st.probe_route == ROUTES[route][2], (st.probe_route, route)
    assert got.NumRows() == want.NumRows() and H.rows_equal_unordered(got, want)
    # the outer filter is evaluated on every probe row
    w = sum(R.str_to_int(c, R.CTX_SELECT)[1] & R.TRUNC_WARN for c in probe.columns[1]._vals if c is not None)
    assert w > 100 and st.str_truncated_warnings == w, (st.str_truncated_warnings, w)


def num_tables(seed, nb=5000, npr=20_000):
    rng = np.random.default_rng(seed)
    build = Chunk([Column(abi.I64, np.arange(nb, dtype=np.int64)), Column(abi.I64, rng.integers(-2, 3, nb))])
    probe = Chunk([Column(abi.I64, rng.integers(-500, nb + 500, npr)), Column(abi.I64, rng.integers(-2, 3, npr), rng.random(npr) > 0.05)])
    return build, probe


# joined row (probe is left): probe k0 y1 | build k2 x3
NY, NX = E.Column(1, abi.I64), E.Column(3, abi.I64)


@pytest.mark.parametrize("route", sorted(ROUTES))
def test_string_constants_in_condition_and_outer_filter_on_every_route(ctx, orc, route):
    build, probe = num_tables(11)
    keep = []
    # OtherCondition IF(build.x > 0, "12abc", "0x"): 12 (a truncation) or 0 (a truncation) — the oracle's Int twin is build.x > 0
    cond = F("if", F("gt", NX, E.Constant(0)), E.Constant("12abc"), E.Constant("0x"))
    cfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1, [cond], (), keep)
    ocfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1, [F("gt", NX, E.Constant(0))], (), keep)
    want = orc.hash_join(ocfg, build, probe)
    got, st = run(ctx, cfg, build, probe, route)
    assert st.probe_route == ROUTES[route][2], (st.probe_route, route)
    assert got.NumRows() == want.NumRows() > 1000 and H.rows_equal_unordered(got, want)
    plain = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1)
    pairs = orc.hash_join(plain, build, probe).NumRows()  # every key-matching pair converts one string with a truncation warning
    assert st.str_truncated_warnings == pairs and st.str_overflow_warnings == 0, (st.str_truncated_warnings, pairs)
    # left outer join, outer filter IF(probe.y > 0, "3z", "0"): the Int twin is probe.y > 0 (NULL y: "0", and an Int NULL — unselected)
    filt = F("if", F("gt", NY, E.Constant(0)), E.Constant("3z"), E.Constant("0"))
    cfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1, (), [filt], keep)
    ocfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1, (), [F("gt", NY, E.Constant(0))], keep)
    want = orc.hash_join(ocfg, build, probe)
    got, st = run(ctx, cfg, build, probe, route)
    assert st.probe_route == ROUTES[route][2], (st.probe_route, route)
    assert got.NumRows() == want.NumRows() and H.rows_equal_unordered(got, want)
    y, ynn = probe.columns[1].data, probe.columns[1].notnull
    w = int(np.sum(ynn & (y > 0)))  # "3z" truncates, "0" does not
    assert st.str_truncated_warnings == w, (st.str_truncated_warnings, w)


@pytest.mark.parametrize("route", sorted(ROUTES))
@pytest.mark.parametrize("where", ["condition", "outer_filter"])
def test_any_failing_row_fails_the_join(ctx, route, where):
    # the documented divergence: the reference reports the error of the last row of a chunk / of a probe row's candidates,
    # which depends on chunk boundaries and hash-chain order; the library fails iff any row or pair it evaluated raised a conversion error.
    # Here only the pairs / rows with x <= 0 (resp. y <= 0) overflow, and they sit anywhere — never only at the end
    build, probe = num_tables(9)
    big = BIG.decode()
    keep = []
    if where == "condition":
        cfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1, [F("if", F("gt", NX, E.Constant(0)), E.Constant("1"), E.Constant(big))], (), keep)
    else:
        cfg = H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1, (), [F("if", F("gt", NY, E.Constant(0)), E.Constant("1"), E.Constant(big))], keep)
    with pytest.raises(_lib.TsqError) as ex:
        run(ctx, cfg, build, probe, route)
    assert ex.value.status == abi.ERR_OVERFLOW_BIGINT


def test_any_failing_string_cell_fails_the_join(ctx):
    # the same with the overflowing value in a string column, in the middle of the probe side, on a key that matches (build keys 0 .. 4999)
    build, probe = tables(9, extra=(1234, BIG))
    probe.columns[0].data[1234] = 100
    keep = []
    for cfg in (H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_INNER, 1, [PS], (), keep),
                H.join_cfg(probe.types(), build.types(), [0], [0], abi.JOIN_LEFT_OUTER, 1, (), [PS], keep)):
        with pytest.raises(_lib.TsqError) as ex:
            run(ctx, cfg, build, probe, "direct")
        assert ex.value.status == abi.ERR_OVERFLOW_BIGINT
