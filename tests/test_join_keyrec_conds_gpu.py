"""GPU parity: OtherConditions on the KEY-RECORD route (csrc/tsq_keyrec.h, k_kr_probe<VERIFY, COND>).  A join on (bigint, varstring) keys
with conditions used to fall back to the direct route; now the probe kernel evaluates them on every key-equal candidate, in the lane
that owns the probe record (joiner.go:155-167), and an outer row whose candidates all fail is NULL-padded once (joiner.go:252-281).
Every case FORCES the radix routes and asserts tsq_stats.probe_route.

The oracle's join evaluates conditions over 8-byte cells only, so a condition over the string payload t has a twin: both sides carry
rank(t), the dense rank of the cell under byte order (NULL for NULL); the GPU runs lt(probe.t, build.t), the oracle lt(probe.rank,
build.rank).  Warning counts come from orc.filter_eval over the candidates of the condition-free join."""
import ctypes as C
import functools

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column, StrColumn, chunk_from_buffers, concat, make_cols, out_buffers

from . import gpu_helpers as G
from . import helpers as H

pytestmark = pytest.mark.gpu
FORCE, OFF = abi.RADIX_FORCE, abi.RADIX_OFF
F = E.ScalarFunction
NB, NP = 9_000, 30_001
WORDS = [b"w%03d" % i for i in range(60)] + [b"", b"a", b"a\x00"]
LONG = {w: w * 9 for w in WORDS[::3]}  # digest form: every third word nine times over (36 bytes: no 32-byte record holds it)


def _side(rng, n, kmax, fvals, tmod, tnull, big_v_at=None):
    k = Column(abi.I64, rng.integers(0, kmax, n), rng.random(n) > 0.02)
    s = [None if rng.random() < 0.03 else WORDS[int(i)] for i in rng.integers(0, len(WORDS), n)]
    v = rng.integers(-9, 10, n).astype(np.int64)
    if big_v_at is not None:
        v[np.arange(n) % 50 == big_v_at] = 1 << 62
    vc = Column(abi.I64, v, rng.random(n) > 0.10)
    f = Column(abi.F64, fvals(rng, n), rng.random(n) > 0.05)
    t = [None if i % tnull == 0 else b"pay%d" % (i % tmod) for i in range(n)]
    return k, s, vc, f, t


def _with_ranks(k, s, v, f, t, rank, long_keys):
    r = Column(abi.I64, np.array([0 if x is None else rank[x] for x in t], np.int64), np.array([x is not None for x in t]))
    if long_keys:
        s = [None if w is None else LONG.get(w, w) for w in s]
    return Chunk([k, StrColumn(s), v, f, StrColumn(t), r])


@functools.lru_cache(maxsize=None)
def fixture_a(long_keys=False, overflow=False):
    """build 9 000 rows / probe 30 001 rows of (k, s, v, f, t, rank(t)); keys (k, s).  overflow: v = 2^62 on build rows i % 50 == 7 and
    probe rows i % 50 == 3 (v + v' overflows BIGINT on their pairs)"""
    rng = np.random.default_rng(404)
    b = _side(rng, NB, 20, lambda r, n: r.integers(0, 4, n).astype(np.float64), 97, 11, 7 if overflow else None)
    p = _side(rng, NP, 24, lambda r, n: r.integers(-50, 50, n).astype(np.float64), 89, 13, 3 if overflow else None)
    rank = {w: i for i, w in enumerate(sorted({x for x in b[4] + p[4] if x is not None}))}
    return _with_ranks(*b, rank, long_keys), _with_ranks(*p, rank, long_keys)


# joined row, probe = left child: probe k0 s1 v2 f3 t4 r5 | build k6 s7 v8 f9 t10 r11 (build = left child: the sides swap places)
def _conds(name, probe_is_left=True):
    po, bo = (0, 6) if probe_is_left else (6, 0)
    pv, bv = E.Column(po + 2, abi.I64), E.Column(bo + 2, abi.I64)
    pf, bf = E.Column(po + 3, abi.F64), E.Column(bo + 3, abi.F64)
    pt, bt = E.Column(po + 4, abi.BYTES), E.Column(bo + 4, abi.BYTES)
    pr, br = E.Column(po + 5, abi.I64), E.Column(bo + 5, abi.I64)
    gpu = {
        "v_sum_gt_5": [F("gt", F("plus", pv, bv), E.Constant(5))],
        "f_div_gt_1": [F("gt", F("div", pf, bf), E.Constant(1.0))],
        "v_sum_gt_0_and_str_lt": [F("gt", F("plus", pv, bv), E.Constant(0)), F("lt", pt, bt)],
        "str_lt": [F("lt", pt, bt)],
        "probe_v_gt_0": [F("gt", pv, E.Constant(0))],
        "constant_false": [F("gt", E.Constant(0), E.Constant(1))],
        "v_sum_gt_17": [F("gt", F("plus", pv, bv), E.Constant(17))],
    }[name]
    twin = {"v_sum_gt_0_and_str_lt": [F("gt", F("plus", pv, bv), E.Constant(0)), F("lt", pr, br)], "str_lt": [F("lt", pr, br)]}.get(name, gpu)
    return gpu, twin


def _cfgs(build, probe, name, jt=abi.JOIN_INNER, inner=1, filters=(), keep=None, **kw):
    gpu, twin = _conds(name, probe_is_left=inner == 1) if name else ((), ())
    left, right = (probe, build) if inner == 1 else (build, probe)
    mk = lambda c: H.join_cfg(left.types(), right.types(), [0, 1], [0, 1], jt, inner, c, filters, keep, **kw)  # noqa: E731
    return mk(gpu), mk(twin)


@functools.lru_cache(maxsize=None)
def _candidates(long_keys=False):
    from oracle import binding as orc
    build, probe = fixture_a(long_keys)
    return orc.hash_join(_cfgs(build, probe, None)[0], build, probe)


def _run(ctx, cfg, build, probe, **kw):
    stats = []
    kw.setdefault("chunk_rows", 4096)
    kw.setdefault("pull_rows", 1 << 16)
    got = G.run_join(ctx, cfg, build, probe, radix=kw.pop("radix", FORCE), stats_out=stats, **kw)
    return got, stats[0]


# ------------------------------------------------------------------ 1. inner joins
@pytest.mark.parametrize("name", ["v_sum_gt_5", "f_div_gt_1", "v_sum_gt_0_and_str_lt", "str_lt", "probe_v_gt_0", "constant_false"])
def test_inner_join_conditions_on_key_records(ctx, orc, name):
    build, probe = fixture_a()
    keep = []
    cfg, ocfg = _cfgs(build, probe, name, keep=keep, probe_batch_rows=12_000)
    assert _candidates().NumRows() > 100_000
    want = orc.hash_join(ocfg, build, probe)
    got, st = _run(ctx, cfg, build, probe)
    assert st.probe_route == abi.ROUTE_KEYREC and st.radix_batches >= 3, (st.probe_route, st.radix_batches)
    assert st.keyrec_digests == 0
    assert got.NumRows() == want.NumRows() and H.rows_equal_unordered(got, want)
    assert (want.NumRows() == 0) == (name == "constant_false") and want.NumRows() < _candidates().NumRows()


def test_inner_join_conditions_with_the_build_side_as_the_left_child(ctx, orc):
    build, probe = fixture_a()
    keep = []
    cfg, ocfg = _cfgs(build, probe, "v_sum_gt_0_and_str_lt", inner=0, keep=keep, probe_batch_rows=12_000)
    want = orc.hash_join(ocfg, build, probe)
    got, st = _run(ctx, cfg, build, probe)
    assert st.probe_route == abi.ROUTE_KEYREC and st.radix_batches >= 3
    assert got.NumRows() == want.NumRows() > 10_000 and H.rows_equal_unordered(got, want)


# ------------------------------------------------------------------ 2. outer joins, with selected[] and an outer-side filter
@pytest.mark.parametrize("jt,inner", [(abi.JOIN_LEFT_OUTER, 1), (abi.JOIN_RIGHT_OUTER, 0)])
@pytest.mark.parametrize("with_selected,with_filter", [(False, False), (True, False), (False, True), (True, True)])
@pytest.mark.parametrize("name", ["v_sum_gt_5", "str_lt"])
def test_outer_join_conditions_on_key_records(ctx, orc, jt, inner, with_selected, with_filter, name):
    build, probe = fixture_a()
    sel = (np.random.default_rng(11).random(NP) > 0.3).astype(np.uint8) if with_selected else None
    filters = [F("gt", E.Column(3, abi.F64), E.Constant(0.25))] if with_filter else ()  # probe.f > 0.25, over the probe schema
    keep = []
    cfg, ocfg = _cfgs(build, probe, name, jt, inner, filters, keep, probe_batch_rows=12_000)
    want = orc.hash_join(ocfg, build, probe, selected=sel)
    got, st = _run(ctx, cfg, build, probe, selected=sel)
    assert st.probe_route == abi.ROUTE_KEYREC, st.probe_route
    assert got.NumRows() == want.NumRows() >= NP and H.rows_equal_unordered(got, want)
    if name == "v_sum_gt_5" and not with_selected and not with_filter:
        # outer rows that HAD candidates and lost them all to the conditions: padded rows beyond those of the condition-free join
        plain = orc.hash_join(_cfgs(build, probe, None, jt, inner)[0], build, probe)
        padded = lambda ch: int(np.count_nonzero(~ch.columns[6 if inner == 1 else 0].notnull))  # noqa: E731  (the build side's k: NULL on a padded row only)
        assert padded(want) - padded(plain) > 5_000


# ------------------------------------------------------------------ 3. warnings are counted once per candidate
@pytest.mark.parametrize("jt", [abi.JOIN_INNER, abi.JOIN_LEFT_OUTER])
def test_division_by_zero_warnings_once_per_candidate(ctx, orc, jt):
    build, probe = fixture_a()
    keep = []
    cfg, _ = _cfgs(build, probe, "f_div_gt_1", jt, keep=keep, probe_batch_rows=12_000)
    _, _, want_w = orc.filter_eval(E.compile_list(_conds("f_div_gt_1")[0]), 1, _candidates())
    assert want_w > 10_000
    want = orc.hash_join(cfg, build, probe)
    got, st = _run(ctx, cfg, build, probe)
    assert st.probe_route == abi.ROUTE_KEYREC
    assert got.NumRows() == want.NumRows() and H.rows_equal_unordered(got, want)
    assert st.div_by_zero_warnings == want_w, (st.div_by_zero_warnings, want_w)
    got0, st0 = _run(ctx, cfg, build, probe, radix=OFF)
    assert st0.probe_route == abi.ROUTE_DIRECT and st0.div_by_zero_warnings == want_w and got0.NumRows() == want.NumRows()


def test_string_valued_condition_warns_once_per_candidate(ctx, orc):
    build, probe = fixture_a()
    keep = []
    bv = E.Column(8, abi.I64)
    cond = F("if", F("gt", bv, E.Constant(0)), E.Constant("12abc"), E.Constant("0x"))  # 12 or 0, a truncation either way; NULL v: "0x"
    left, right = probe, build
    cfg = H.join_cfg(left.types(), right.types(), [0, 1], [0, 1], abi.JOIN_INNER, 1, [cond], (), keep, probe_batch_rows=12_000)
    ocfg = H.join_cfg(left.types(), right.types(), [0, 1], [0, 1], abi.JOIN_INNER, 1, [F("gt", bv, E.Constant(0))], (), keep)
    want = orc.hash_join(ocfg, build, probe)
    got, st = _run(ctx, cfg, build, probe)
    assert st.probe_route == abi.ROUTE_KEYREC
    assert got.NumRows() == want.NumRows() > 10_000 and H.rows_equal_unordered(got, want)
    assert st.str_truncated_warnings == _candidates().NumRows() and st.str_overflow_warnings == 0, (st.str_truncated_warnings, _candidates().NumRows())


# ------------------------------------------------------------------ 4. digest records: a candidate whose bytes differ never reaches the conditions
@pytest.mark.parametrize("weak_digests", [False, True])
@pytest.mark.parametrize("jt", [abi.JOIN_INNER, abi.JOIN_LEFT_OUTER])
def test_conditions_behind_the_byte_comparison_of_digest_records(ctx, orc, jt, weak_digests):
    build, probe = fixture_a(long_keys=True)
    assert _candidates(True).NumRows() == _candidates().NumRows()
    keep = []
    cfg, _ = _cfgs(build, probe, "f_div_gt_1", jt, keep=keep, probe_batch_rows=12_000)
    _, _, want_w = orc.filter_eval(E.compile_list(_conds("f_div_gt_1")[0]), 1, _candidates(True))
    want = orc.hash_join(cfg, build, probe)
    with ctx.knobs(**({"KEYREC": 3} if weak_digests else {})):  # KEYREC = 3: every two cells of one length are candidates of one another
        got, st = _run(ctx, cfg, build, probe)
        assert st.probe_route == abi.ROUTE_KEYREC and st.keyrec_digests == 1, (st.probe_route, st.keyrec_digests)
        assert got.NumRows() == want.NumRows() and H.rows_equal_unordered(got, want)
        assert st.div_by_zero_warnings == want_w > 10_000, (st.div_by_zero_warnings, want_w)
        if jt == abi.JOIN_INNER:
            c, cst = _run(ctx, cfg, build, probe, count_only=True)
            assert cst.probe_route == abi.ROUTE_KEYREC and c == want.NumRows() and cst.div_by_zero_warnings == want_w


# ------------------------------------------------------------------ 5. COUNT(*)
@pytest.mark.parametrize("name", ["v_sum_gt_5", "f_div_gt_1", "v_sum_gt_0_and_str_lt"])
def test_count_with_conditions_on_key_records(ctx, orc, name):
    build, probe = fixture_a()
    keep = []
    cfg, ocfg = _cfgs(build, probe, name, keep=keep, probe_batch_rows=12_000)
    want = orc.hash_join(ocfg, build, probe).NumRows()
    c, st = _run(ctx, cfg, build, probe, count_only=True)
    assert st.probe_route == abi.ROUTE_KEYREC and st.radix_batches >= 3, (st.probe_route, st.radix_batches)
    assert c == want > 10_000
    want_w = orc.filter_eval(E.compile_list(_conds(name)[1]), len(_conds(name)[1]), _candidates())[2]
    assert st.div_by_zero_warnings == want_w and (want_w > 10_000) == (name == "f_div_gt_1")
    assert st.str_truncated_warnings == 0 and st.str_overflow_warnings == 0


# ------------------------------------------------------------------ 6. a condition that raises an error: the direct route reports it
def _error_of(ctx, cfg, build, probe, **kw):
    with pytest.raises(_lib.TsqError) as ex:
        _run(ctx, cfg, build, probe, **kw)
    return ex.value.status, ex.value.message


@pytest.mark.parametrize("count_only", [False, True])
def test_overflow_in_a_condition_fails_as_on_the_direct_route(ctx, orc, count_only):
    build, probe = fixture_a(overflow=True)
    keep = []
    cfg, _ = _cfgs(build, probe, "v_sum_gt_5", keep=keep, probe_batch_rows=12_000)
    with pytest.raises(orc.OracleError) as oex:
        orc.hash_join(cfg, build, probe)
    assert oex.value.status == abi.ERR_OVERFLOW_BIGINT
    direct = _error_of(ctx, cfg, build, probe, radix=OFF, count_only=count_only)
    assert direct[0] == abi.ERR_OVERFLOW_BIGINT
    assert _error_of(ctx, cfg, build, probe, count_only=count_only) == direct


def test_a_clean_batch_is_delivered_before_the_failing_one(ctx, orc):
    build, probe_ovf = fixture_a(overflow=True)
    _, probe_ok = fixture_a()
    first, second = probe_ok.slice(0, 12_032), probe_ovf.slice(12_032, 24_064)  # (a device batch is a multiple of 64 rows: one push fills it)
    keep = []
    cfg, _ = _cfgs(build, first, "v_sum_gt_5", keep=keep, probe_batch_rows=12_032)
    # (the build side's 2^62 cells alone overflow nothing: -9 <= probe.v <= 9 in the first batch)
    want_first = orc.hash_join(cfg, build, first)
    assert want_first.NumRows() > 1_000
    with pytest.raises(orc.OracleError):
        orc.hash_join(cfg, build, second)
    lib = ctx.lib
    h = C.c_void_p()
    _lib.check(lib.tsq_join_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
    try:
        _lib.check(lib.tsq_join_set_radix(h, FORCE), h)
        G.push_chunked(lib.tsq_join_build_push, h, build, 1 << 20)
        _lib.check(lib.tsq_join_build_finish(h), h)
        out_types = probe_ok.types() + build.types()
        got = []

        def pull_all():
            while True:
                k2 = []
                pn, pb = C.c_int64(0), (C.c_int64 * len(out_types))()
                _lib.check(lib.tsq_join_peek(h, 1 << 16, C.byref(pn), pb, len(out_types)), h)
                out, bufs = out_buffers(out_types, 1 << 16, k2, list(pb))
                n, eos = C.c_int64(0), C.c_int32(0)
                _lib.check(lib.tsq_join_pull(h, out, len(out_types), 1 << 16, C.byref(n), C.byref(eos)), h)
                if n.value == 0:
                    return
                got.append(chunk_from_buffers(out_types, bufs, n.value))

        def push(part):
            k2 = []
            _lib.check(lib.tsq_join_probe_push(h, make_cols(part.columns, k2), len(part.columns), part.NumRows(), None), h)
            ctx.sync()  # (a pull finds a batch whose copies are still on the way "not there yet")
            pull_all()
        push(first)
        st = abi.Stats()
        _lib.check(lib.tsq_join_stats(h, C.byref(st)), h)
        assert st.probe_route == abi.ROUTE_KEYREC and st.radix_batches == 1
        rows = concat(got, out_types)
        assert rows.NumRows() == want_first.NumRows() and H.rows_equal_unordered(rows, want_first)
        with pytest.raises(_lib.TsqError) as ex:
            push(second)
            _lib.check(lib.tsq_join_probe_finish(h), h)
            pull_all()
        assert ex.value.status == abi.ERR_OVERFLOW_BIGINT
    finally:
        lib.tsq_join_destroy(h)


# ------------------------------------------------------------------ 7. a hot key: 5 000 build rows under one (k, s), no pair passes
def test_hot_key_whose_candidates_all_fail(ctx, orc):
    rng = np.random.default_rng(9)
    nb, npr = 12_000, 20_000

    def side(n, kmax, hot_rows):
        k = rng.integers(0, kmax, n)
        s = [WORDS[int(i)] for i in rng.integers(0, 60, n)]
        for i in hot_rows:
            k[i], s[i] = 777, b"hot"
        return Chunk([Column(abi.I64, k), StrColumn(s), Column(abi.I64, rng.integers(-9, 10, n), rng.random(n) > 0.1)])
    build = side(nb, 20, rng.choice(nb, 5_000, replace=False).tolist())
    probe = side(npr, 24, rng.choice(npr, 40, replace=False).tolist())
    pv, bv = E.Column(2, abi.I64), E.Column(5, abi.I64)
    keep = []
    cfg = H.join_cfg(probe.types(), build.types(), [0, 1], [0, 1], abi.JOIN_LEFT_OUTER, 1, [F("gt", F("plus", pv, bv), E.Constant(17))], (), keep)
    plain = H.join_cfg(probe.types(), build.types(), [0, 1], [0, 1], abi.JOIN_INNER, 1)
    assert orc.hash_join(plain, build, probe).NumRows() > 200_000
    want = orc.hash_join(cfg, build, probe)
    got, st = _run(ctx, cfg, build, probe, chunk_rows=1 << 20)
    assert st.probe_route == abi.ROUTE_KEYREC, st.probe_route
    assert got.NumRows() == want.NumRows() >= npr and H.rows_equal_unordered(got, want)


# ------------------------------------------------------------------ 8. the knob
def test_knob_keeps_joins_with_conditions_on_the_direct_route(ctx, orc):
    build, probe = fixture_a()
    keep = []
    cfg, ocfg = _cfgs(build, probe, "v_sum_gt_0_and_str_lt", abi.JOIN_LEFT_OUTER, keep=keep, probe_batch_rows=12_000)
    want = orc.hash_join(ocfg, build, probe)
    with ctx.knobs(KEYREC_CONDS=0):
        got0, st0 = _run(ctx, cfg, build, probe)
        c0, cst0 = _run(ctx, _cfgs(build, probe, "v_sum_gt_5", keep=keep)[0], build, probe, count_only=True)
    assert st0.probe_route == abi.ROUTE_DIRECT and cst0.probe_route == abi.ROUTE_DIRECT
    got1, st1 = _run(ctx, cfg, build, probe)
    assert st1.probe_route == abi.ROUTE_KEYREC
    assert got0.NumRows() == got1.NumRows() == want.NumRows() and H.rows_equal_unordered(got0, want) and H.rows_equal_unordered(got1, want)
    assert c0 == orc.hash_join(_cfgs(build, probe, "v_sum_gt_5", keep=keep)[0], build, probe).NumRows()


# ------------------------------------------------------------------ 9. the reference's own vectors that carry OtherConditions
# tests/golden/join_cases.json joins on ONE integer column; on (k, k') with k' a copy of k the same rows join and the key no longer packs
# into one word (test_join_keyrec_gpu.test_golden_join_cases_on_two_key_columns) — here for the cases WITH conditions, route asserted:
# join_test.go:112-116's a.c1 + b.c1 > 5 runs inside the probe kernel
@pytest.mark.parametrize("case", [c for c in H.golden("join_cases.json") if c.get("other_conds")], ids=lambda c: c["ref"][:48])
def test_golden_join_cases_with_conditions_on_two_key_columns(ctx, case):
    keep = []
    _, left, right, _, _, conds, filt = H.lower_join_case(case, keep)
    lk, rk = case["left_keys"][0], case["right_keys"][0]

    def widen(chk, kc):
        c = chk.columns[kc]
        return Chunk(list(chk.columns) + [Column(c.tp, c.data.copy(), None if c.notnull is None else c.notnull.copy())])
    left2, right2 = widen(left, lk), widen(right, rk)
    nl, nr = len(left.columns), len(right.columns)

    def shift(e):  # conditions address left || right: the right side's columns moved one place to the right
        if isinstance(e, E.Column):
            return E.Column(e.index + 1, e.tp) if e.index >= nl else e
        if isinstance(e, E.ScalarFunction):
            return F(e.name, *[shift(a) for a in e.args])
        return e
    inner = case["inner_child"]
    cfg = H.join_cfg(left2.types(), right2.types(), [lk, nl], [rk, nr], H.JOIN_TYPES[case["type"]], inner, [shift(c) for c in conds], filt, keep)
    build, probe = (right2, left2) if inner == 1 else (left2, right2)
    stats = []
    got = G.run_join(ctx, cfg, build, probe, radix=FORCE, stats_out=stats)
    want = []
    for row in case["expect"]:
        l, r = list(row[:nl]), list(row[nl:])
        want.append(tuple(l + [l[lk]] + r + [r[rk]]))
    assert H.rows_equal_unordered(got, want), case["ref"]
    if len(case["left"]) and len(case["right"]):
        assert stats[0].probe_route == abi.ROUTE_KEYREC, (case["ref"], stats[0].probe_route)
