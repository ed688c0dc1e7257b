"""GPU: the edge-value groups of tests/agg_edge.py on every route an aggregate can take through tsq_agg.hip and its headers, each result
checked against the exact verdict of agg_edge.expected (pinned on the CPU oracle by tests/test_agg_edge_cpu.py).

The table.  One per (argument type, size): key k = 0 .. E-1 carries edge group k of that type, filler groups with ordinary random
cells (H.random_column's ranges) bring it to the size at which a route engages — 2 048 rows / 40 groups for the row path, L mode,
the dictionary, the group-id front and the stream aggregate; 70 016 rows / 5 000 groups (est_groups = 5 000) for H mode, the packed
route and the partitioned groups.  The table is two halves: cell j of an edge group lies in half j mod 2, each half is shuffled with
a fixed seed.  With AGG_BATCH_ROWS = half a table every edge group of two cells or more is therefore split over two device batches
(run_route asserts it for every batch-splitting route), and the two halves are the inputs of the Partial1 stages of the Partial1 -> Final tests (the half-sums of every integer group fit
BIGINT by this construction: a partial SUM is a BIGINT column, so a half that overflows is an error of the plan, not of the route).
"late" tables keep every edge cell in the second half: the first batch shows the packed route small non-negative values only, so
the argument column travels as 16- or 32-bit cells and the edge values arrive as exception rows.
"straddle" tables serve the batch-splitting variants of the stream aggregate, whose rows arrive ordered by key: a device batch is
1 024 rows at the least, so runs of filler groups pad the table until a multiple of 1 024 falls INSIDE every edge group of two cells
or more (one batch boundary per group, about 20 000 rows) — the group is open when a batch ends and row 0 of the next batch is no head.

Plans.  The LDS routes hold at most 5 words per group and the lane route of the stream aggregate 4 reducing aggregates, so the
functions are split over plan A = FIRST_ROW(key), COUNT(arg), MIN(arg), MAX(arg) and plan B = FIRST_ROW(key), SUM(arg), AVG(arg)
(U64 arguments: plan A only).  Groups whose exact integer sum leaves BIGINT are errors of plan B: they run in tables of their own
(test_error_groups_*), plan A sees them in the main table.  The hot-key words of the packed route (s_hw, tsq_daagg.h) hold plans of
at most 3 words (TSQ_DAAGG_HOT_MAXW): plan A, plan B over reals, and the one-function plans SUM and AVG over integers, which the two
hot-key routes therefore run as well (plan B over integers, 5 words, travels through the partitioned store on every route).

Rules pinned here (DESIGN.md "Aggregates at the edge values"): MIN / MAX of reals order the cells by their memcomparable image — a
NaN with the sign bit clear ranks above +inf, one with the sign bit set below -inf, +0.0 above -0.0 — on every route; a real SUM / AVG
is -0.0 iff every non-NULL cell is -0.0."""
import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Chunk, Column, StrColumn, concat
from tinysql_amd.executor import AggFuncDesc, HashAggExec, MockDataSource

from . import agg_edge as AE
from . import gpu_helpers as G
from . import helpers as H
from .test_agg_gpu import out_types_for

pytestmark = pytest.mark.gpu
OFF, FORCE = abi.AGGFAST_OFF, abi.AGGFAST_FORCE
HALF = {"small": 1024, "large": 35_008}   # (multiples of 64: AGG_BATCH_ROWS is rounded up to one)
GROUPS = {"small": 40, "large": 5000}
EST_LARGE = 5000
PLAN_FUNCS = {"A": ("count", "min", "max"), "B": ("sum", "avg"), "SUM": ("sum",), "AVG": ("avg",)}
PLANS_OF = {"i64": ("A", "B"), "u64": ("A",), "f64": ("A", "B"), "f32": ("A", "B")}
TYPE_NAMES = ("i64", "u64", "f64", "f32")


def _is_err(tp, cells):
    return tp == "i64" and AE.expected("sum", tp, cells)[0] == "err"


def designed(tp, plan):
    """the edge groups of the main table of (type, plan): all of them but the error groups of plan B"""
    return [(n, c) for n, c in AE.EDGE_GROUPS[tp] if not (plan != "A" and _is_err(tp, c))]


# ---------------------------------------------------------------------------------------------------------------- tables
class Table:
    """k: group index of every row; arg: the argument Column; cells: {k: the group's cells}; names: {k: edge group name}"""

    def __init__(self, tp, k, arg, cells, names, n_groups, half):
        self.tp, self.k, self.arg, self.cells, self.names, self.n_groups, self.half = tp, k, arg, cells, names, n_groups, half


_NP = {"i64": np.int64, "u64": np.uint64, "f64": np.float64, "f32": np.float32}


def _filler_cells(rng, tp, n, small_max=None):
    if small_max is not None:  # a "late" table: small non-negative values, no NULL — the first batch shows nothing else
        return rng.integers(0, small_max, n).astype(_NP[tp]), np.ones(n, bool)
    nn = rng.random(n) >= 0.2
    if tp in ("f64", "f32"):
        return (rng.random(n) * 1e6 * np.where(rng.random(n) < 0.5, -1.0, 1.0)).astype(_NP[tp]), nn
    if tp == "u64":
        return rng.integers(0, 1 << 64, n, dtype=np.uint64), nn
    return rng.integers(-10**6, 10**6, n).astype(np.int64), nn


def _cells_array(tp, cells):
    nn = np.array([c is not None for c in cells], dtype=bool)
    if tp == "u64":
        data = np.array([0 if c is None else c for c in cells], dtype=np.uint64)
    elif tp == "i64":
        data = np.array([0 if c is None else c for c in cells], dtype=np.int64)
    else:
        data = np.array([0.0 if c is None else c for c in cells], dtype=np.float64).astype(_NP[tp])
    return data, nn


_TABLES = {}


def make_table(tp, size, groups, layout="alternate", repeat=None, small_max=None):
    """groups: [(name, cells)] -> keys 0 .. E-1; layout "alternate": cell j of a group in half j mod 2, "late": every edge cell in
    the second half; repeat: {name: r} the cells of that group r times over (a hot key); small_max: see _filler_cells"""
    memo = (tp, size, tuple(n for n, _ in groups), layout, tuple(sorted((repeat or {}).items())), small_max)
    if memo in _TABLES:
        return _TABLES[memo]
    rng = np.random.default_rng(len(groups) * 1000 + HALF[size] + 7 * TYPE_NAMES.index(tp) + (small_max or 0) % 97 + len(layout))
    if layout == "straddle":
        t = _straddle_table(rng, tp, groups)
        _check_cells(t)
        _TABLES[memo] = t
        return t
    half, n_groups, E = HALF[size], GROUPS[size], len(groups)
    cells, names = {}, {}
    ek, ec = ([], []), ([], [])  # per half: group index, cell
    for k, (name, c) in enumerate(groups):
        c = list(c) * (repeat or {}).get(name, 1)
        cells[k], names[k] = c, name
        for j, cell in enumerate(c):
            h = 1 if layout == "late" else j % 2
            ek[h].append(k)
            ec[h].append(cell)
    parts_k, parts_d, parts_nn = [], [], []
    for h in (0, 1):
        n_fill = half - len(ek[h])
        assert n_fill > 0, "the edge groups do not fit half a table"
        fk = rng.integers(E, n_groups, n_fill)
        fd, fnn = _filler_cells(rng, tp, n_fill, small_max)
        ed, enn = _cells_array(tp, ec[h])
        perm = rng.permutation(half)
        parts_k.append(np.concatenate([np.array(ek[h], dtype=np.int64), fk])[perm])
        parts_d.append(np.concatenate([ed, fd])[perm])
        parts_nn.append(np.concatenate([enn, fnn])[perm])
    k, d, nn = np.concatenate(parts_k), np.concatenate(parts_d), np.concatenate(parts_nn)
    t = Table(tp, k, Column(AE.TYPES[tp], d, nn), cells, names, n_groups, half)
    _check_cells(t)
    _TABLES[memo] = t
    return t


def _check_cells(t):
    """the cells really are in the column, bit for bit (a NaN keeps its sign and payload through numpy)"""
    d, nn = t.arg.data, t.arg.notnull

    def image(x):
        return -1 if x is None else (int(x) if t.tp in ("i64", "u64") else AE.bits_of(float(x), t.tp))
    for kk, c in t.cells.items():
        have = sorted(image(d[i] if nn[i] else None) for i in np.nonzero(t.k == kk)[0])
        assert have == sorted(image(x) for x in c), (t.tp, t.names[kk])


STREAM_BATCH = 1024  # the least device batch (tsq_agg.hip: AGG_BATCH_ROWS below 1024 is taken as 1024)


def _straddle_table(rng, tp, groups):
    """rows in key order; group ids ascend in the order of appearance (edge groups and the filler runs between them); a multiple of
    STREAM_BATCH falls between the first and the second half of the cells of every edge group of two cells or more"""
    seg_k, seg_d, seg_nn = [], [], []
    cells, names = {}, {}
    next_id, pos = 0, 0

    def fillers(n):
        nonlocal next_id, pos
        while n > 0:
            run = min(n, int(rng.integers(1, 90)))
            fd, fnn = _filler_cells(rng, tp, run)
            seg_k.append(np.full(run, next_id, dtype=np.int64))
            seg_d.append(fd)
            seg_nn.append(fnn)
            next_id, pos, n = next_id + 1, pos + run, n - run

    for name, c in groups:
        if len(c) >= 2:
            fillers((-(pos + (len(c) + 1) // 2)) % STREAM_BATCH)
        else:
            fillers(int(rng.integers(1, 40)))
        ed, enn = _cells_array(tp, c)
        seg_k.append(np.full(len(c), next_id, dtype=np.int64))
        seg_d.append(ed)
        seg_nn.append(enn)
        cells[next_id], names[next_id] = list(c), name
        next_id, pos = next_id + 1, pos + len(c)
    fillers(200)
    k = np.concatenate(seg_k)
    return Table(tp, k, Column(AE.TYPES[tp], np.concatenate(seg_d), np.concatenate(seg_nn)), cells, names, next_id, STREAM_BATCH)


# ---- key columns of a table, per kind: (the columns, the value FIRST_ROW(column 0) shows for group index k)
def _spread(k):
    """distinct keys spread over 62 bits (no packed route: multiplication by an odd number is a bijection modulo 2^62)"""
    return (np.asarray(k, dtype=np.uint64) * np.uint64(982_451_653_000_003) % np.uint64(1 << 62)).astype(np.int64)


def key_columns(kind, k):
    if kind == "dense":
        return [Column(abi.I64, k)], lambda x: x
    if kind == "spread":
        return [Column(abi.I64, _spread(k))], lambda x: int(_spread([x])[0])
    if kind == "str":
        return [StrColumn([b"%d" % x for x in k.tolist()])], lambda x: b"%d" % x
    if kind == "two":
        return [Column(abi.I64, k), Column(abi.I64, k % 3 - 1)], lambda x: x
    if kind == "six":  # (the first column identifies the group; the others are functions of it)
        return [Column(abi.I64, k), Column(abi.I64, k % 7), Column(abi.I64, np.full(len(k), 3)), Column(abi.U64, (k % 2).astype(np.uint64)),
                Column(abi.I64, -k), Column(abi.I64, k * 5)], lambda x: x
    raise AssertionError(kind)


def plan_aggs(tp, plan, n_keys, key_type=abi.I64):
    t = AE.TYPES[tp]
    return [(abi.AGG_FIRSTROW, 0, key_type)] + [(AE.FUNC_CODE[f], n_keys, t) for f in PLAN_FUNCS[plan]]


# ---------------------------------------------------------------------------------------------------------------- routes
# size, key kind, fast mode, est_groups, knobs, split (AGG_BATCH_ROWS = half a table, pushed half by half), stream, exec (HashAggExec),
# check(stats), types (default: all four), layout / small_max / repeat of the table
def _r(size, keys="dense", fast=OFF, est=0, knobs=None, split=False, stream=False, check=None, types=TYPE_NAMES, **table_kw):
    return dict(size=size, keys=keys, fast=fast, est=est, knobs=knobs or {}, split=split, stream=stream, check=check, types=types, table_kw=table_kw)


def _lds(st):
    assert st.radix_batches >= 1, st.radix_batches


def _h_mode(st):
    assert st.radix_batches >= 1 and st.packed_key_bits == 0, (st.radix_batches, st.packed_key_bits)


def _packed(dense_flushes, slice_bits=None):
    def check(st):
        assert st.packed_key_bits > 0 and st.dense_flushes == dense_flushes, (st.packed_key_bits, st.dense_flushes)
        if slice_bits is not None:
            assert st.table_slice_bits == slice_bits, st.table_slice_bits
    return check


def _pg(st):
    assert st.build_partitioned == 4, (st.build_partitioned, st.dense_flushes)


def _dict(st):
    assert st.build_partitioned == 3, st.build_partitioned


HOT = {"i64": {"minus_ones": 300}, "u64": {"zero_and_ones": 300}, "f64": {"neg_zero_twice": 300}, "f32": {"neg_zero_twice": 300}}
ROUTES = {
    "row": _r("small"),
    "row_split": _r("small", split=True),
    "two_keys": _r("small", keys="two", knobs={"AGG_WIDE_KEYS": 0}),
    "lds_l": _r("small", fast=FORCE, check=_lds),
    "lds_l_split": _r("small", fast=FORCE, split=True, check=_lds),
    "lds_h": _r("large", keys="spread", fast=FORCE, est=EST_LARGE, check=_h_mode),
    "lds_h_split": _r("large", keys="spread", fast=FORCE, est=EST_LARGE, split=True, check=_h_mode),
    "packed_dense": _r("large", fast=FORCE, est=EST_LARGE, knobs={"AGG_DENSE": 1}, check=_packed(1)),
    "packed_dense_split": _r("large", fast=FORCE, est=EST_LARGE, knobs={"AGG_DENSE": 1}, split=True, check=_packed(1)),
    "packed_no_dense_split": _r("large", fast=FORCE, est=EST_LARGE, knobs={"AGG_DENSE": 0}, split=True, check=_packed(0)),
    "packed_narrow16": _r("large", fast=FORCE, est=EST_LARGE, split=True, check=_packed(1, 16), types=("i64", "u64"), layout="late", small_max=60_000),
    "packed_narrow32": _r("large", fast=FORCE, est=EST_LARGE, split=True, check=_packed(1, 32), types=("i64", "u64"), layout="late", small_max=3_000_000_000),
    # one edge group per type repeated until it holds 8 % of a batch and more (TSQ_DAAGG_HOT_MIN: 0.018 %): with the sampling on (the
    # default) its rows are aggregated in the partition kernel's hot-key words, with it off they overflow their region and take the
    # overflow store.  No statistic names either path; both must give the row path's bits (test_every_route_agrees_*).
    "packed_hot": _r("large", fast=FORCE, est=EST_LARGE, knobs={"DAAGG_HOT": 1}, split=True, check=_packed(1), repeat=HOT),
    "packed_hot_off": _r("large", fast=FORCE, est=EST_LARGE, knobs={"DAAGG_HOT": 0}, split=True, check=_packed(1), repeat=HOT),
    "pg": _r("large", keys="spread", fast=FORCE, knobs={"AGG_PG": 6}, check=_pg),
    "pg_split": _r("large", keys="spread", fast=FORCE, knobs={"AGG_PG": 6}, split=True, check=_pg),
    "pg_small": _r("small", keys="spread", fast=FORCE, knobs={"AGG_PG": 2}, check=_pg),
    # (the dictionary of group keys carries 8-byte argument columns only — tsq_agg.hip `travel` —, so no F32 parametrisation)
    "str_key": _r("small", keys="str", fast=FORCE, check=_dict, types=("i64", "u64", "f64")),
    "six_keys": _r("small", keys="six"),
    "stream_lanes": _r("small", stream=True, knobs={"STREAMAGG_LANES": 1}),
    "stream_lanes_split": _r("small", stream=True, knobs={"STREAMAGG_LANES": 1}, split=True, layout="straddle"),
    "stream_general": _r("small", stream=True, knobs={"STREAMAGG_LANES": 0}),
    "stream_general_split": _r("small", stream=True, knobs={"STREAMAGG_LANES": 0}, split=True, layout="straddle"),
}


def plans_for(route, tp):
    """the plans a route runs over arguments of type tp (see the module's docstring for the hot-key routes)"""
    return PLANS_OF[tp] + (("SUM", "AVG") if route.startswith("packed_hot") and tp == "i64" else ())


def route_table(route, tp, groups):
    kw = dict(ROUTES[route]["table_kw"])
    if "repeat" in kw:
        kw["repeat"] = kw["repeat"][tp]
    return make_table(tp, ROUTES[route]["size"], groups, **kw)


def run_route(ctx, route, tbl, plan):
    """-> {group index k: result row (without the key)} of plan `plan` over table `tbl` on route `route` (a name, or a route itself)"""
    r = ROUTES[route] if isinstance(route, str) else route
    key_cols, key_of = key_columns(r["keys"], tbl.k)
    nk = len(key_cols)
    cols = key_cols + [tbl.arg]
    if r["stream"]:  # StreamAggExec: rows ordered by the key (a stable sort: the rows of a group keep their shuffled order)
        order = np.argsort(tbl.k, kind="stable")
        cols = [Column(c.tp, c.data[order], None if c.notnull is None else c.notnull[order]) for c in cols]
        pushed_k = tbl.k[order]
    else:
        pushed_k = tbl.k
    if r["split"] and r["table_kw"].get("layout") != "late":  # every edge group of two cells or more lies in two device batches
        for k, c in tbl.cells.items():
            assert len(c) < 2 or len(set((np.nonzero(pushed_k == k)[0] // tbl.half).tolist())) >= 2, (tbl.names[k], tbl.half)
    chk = Chunk(cols)
    types = chk.types()
    aggs = plan_aggs(tbl.tp, plan, nk, types[0])
    knobs = dict(r["knobs"])
    if r["split"]:
        knobs["AGG_BATCH_ROWS"] = tbl.half
    chunk_rows = tbl.half if r["split"] else 1 << 22
    stats = []
    with ctx.knobs(**knobs):
        if r["keys"] == "six":  # more than four key columns: tsq_agg_create_keys, through the executor
            exe = HashAggExec(ctx, MockDataSource(ctx, chk, 1024), list(range(nk)), [AggFuncDesc(a[0], a[1], a[2]) for a in aggs])
            exe.Open()
            out = []
            try:
                while True:
                    c = exe.Next()
                    if c.NumRows() == 0:
                        break
                    out.append(c)
            finally:
                exe.Close()
            got = concat(out, exe.Schema())
        else:
            cfg = H.agg_cfg(types, list(range(nk)), aggs, est_groups=r["est"])
            got = G.run_agg(ctx, cfg, chk, out_types_for(aggs), chunk_rows=chunk_rows, pull_rows=1 << 16, fast=None if r["stream"] else r["fast"],
                            stats_out=stats, stream=r["stream"])
    if r["check"] is not None:
        r["check"](stats[0])
    back = {key_of(k): k for k in range(tbl.n_groups)}
    rows = {back[row[0]]: row[1:] for row in got.rows()}
    assert len(rows) == got.NumRows() == len(set(tbl.k.tolist())), (got.NumRows(), len(rows))
    return rows


def compare(tbl, plan, rows, where):
    """every edge group of the table against its verdict; returns how many groups were compared"""
    compared = 0
    for k, cells in tbl.cells.items():
        for col, func in enumerate(PLAN_FUNCS[plan]):
            wrong = AE.satisfies(AE.expected(func, tbl.tp, cells), rows[k][col], tbl.tp)
            assert wrong == "", "%s: %s(%s) of group %r: %s" % (where, func, tbl.tp, tbl.names[k], wrong)
        compared += 1
    return compared


CASES = [(route, tp) for route in ROUTES for tp in ROUTES[route]["types"]]


@pytest.mark.parametrize("route,tp", CASES, ids=["%s-%s" % c for c in CASES])
def test_edge_groups_on_every_route(ctx, route, tp):
    for plan in plans_for(route, tp):
        groups = designed(tp, plan)
        tbl = route_table(route, tp, groups)
        rows = run_route(ctx, route, tbl, plan)
        assert compare(tbl, plan, rows, route) == len(groups) == len(AE.EDGE_GROUPS[tp]) - (2 if tp == "i64" and plan != "A" else 0)


ERR_ROUTES = [r for r in ROUTES if "i64" in ROUTES[r]["types"]]


@pytest.mark.parametrize("route", ERR_ROUTES)
def test_error_groups_raise_and_the_same_table_without_them_does_not(ctx, route):
    """a group whose exact final sum leaves BIGINT fails SUM and AVG alike (AVG's own emit code included), on every route; the same
    table without the group succeeds"""
    base = designed("i64", "B")
    errs = [(n, c) for n, c in AE.EDGE_GROUPS["i64"] if _is_err("i64", c)]
    assert [n for n, _ in errs] == ["final_over", "final_under"]
    for plan in ("SUM", "AVG"):
        for g in errs:
            tbl = route_table(route, "i64", base + [g])
            with pytest.raises(_lib.TsqError) as ei:
                run_route(ctx, route, tbl, plan)
            assert ei.value.status == abi.ERR_OVERFLOW_BIGINT, (plan, g[0])
        tbl = route_table(route, "i64", base)
        assert compare(tbl, plan, run_route(ctx, route, tbl, plan), route) == len(base)


# ---------------------------------------------------------------------------------------------------------------- no GROUP BY
@pytest.mark.parametrize("stream", [False, True], ids=["hash", "stream"])
@pytest.mark.parametrize("tp", TYPE_NAMES)
def test_every_edge_group_alone_as_a_scalar_aggregate(ctx, tp, stream):
    t = AE.TYPES[tp]
    compared = 0
    for name, cells in AE.EDGE_GROUPS[tp]:
        chk = H.chunk_from_rows([[c] for c in cells], [t])
        for func in AE.FUNCS_OF[tp]:
            aggs = [(AE.FUNC_CODE[func], 0, t)]
            verdict = AE.expected(func, tp, cells)
            if verdict[0] == "err":
                with pytest.raises(_lib.TsqError) as ei:
                    G.run_agg(ctx, H.agg_cfg([t], [], aggs), chk, out_types_for(aggs), stream=stream)
                assert ei.value.status == verdict[1], (name, func)
                continue
            out = G.run_agg(ctx, H.agg_cfg([t], [], aggs), chk, out_types_for(aggs), stream=stream)
            assert out.NumRows() == 1
            wrong = AE.satisfies(verdict, out.rows()[0][0], tp)
            assert wrong == "", "%s(%s) of group %r alone: %s" % (func, tp, name, wrong)
        compared += 1
    assert compared == len(AE.EDGE_GROUPS[tp])


# ---------------------------------------------------------------------------------------------------------------- Partial1 -> Final
def _partial_final(ctx, tbl, plan, stream, orc):
    t = AE.TYPES[tbl.tp]
    chk = Chunk([Column(abi.I64, tbl.k), tbl.arg])
    types = [abi.I64, t]
    full = plan_aggs(tbl.tp, plan, 1)
    paggs = [(f, c, tp_, abi.MODE_PARTIAL1) for f, c, tp_ in full]
    pt = out_types_for(paggs)
    parts = []
    for lo in (0, tbl.half):
        part = chk.slice(lo, lo + tbl.half)
        if stream:
            part = orc.sort_rows(part, [0], [False])
        parts.append(G.run_agg(ctx, H.agg_cfg(types, [0], paggs), part, pt, chunk_rows=1 << 22, pull_rows=1 << 16, stream=stream))
    both = concat(parts, pt)
    if stream:
        both = orc.sort_rows(both, [0], [False])
    faggs, col = [(abi.AGG_FIRSTROW, 0, abi.I64, abi.MODE_FINAL)], 1
    for f, _, tp_ in full[1:]:
        if f == abi.AGG_AVG:  # partial AVG: (count, sum)
            faggs.append((f, col, pt[col + 1], abi.MODE_FINAL, col + 1))
            col += 2
        else:
            faggs.append((f, col, pt[col] if f != abi.AGG_COUNT else t, abi.MODE_FINAL))
            col += 1
    got = G.run_agg(ctx, H.agg_cfg(pt, [0], faggs), both, out_types_for(full), chunk_rows=1 << 22, pull_rows=1 << 16, stream=stream)
    rows = {row[0]: row[1:] for row in got.rows()}
    assert len(rows) == got.NumRows()
    return rows


@pytest.mark.parametrize("stream", [False, True], ids=["hash", "stream"])
@pytest.mark.parametrize("tp", TYPE_NAMES)
def test_partial1_then_final_over_the_two_halves(ctx, orc, tp, stream):
    for plan in PLANS_OF[tp]:
        groups = designed(tp, plan)
        tbl = make_table(tp, "small", groups)
        rows = _partial_final(ctx, tbl, plan, stream, orc)
        assert compare(tbl, plan, rows, "partial->final") == len(groups)


# ---------------------------------------------------------------------------------------------------------------- agreement
def _exact_image(tp, plan, row):
    """the columns that must be bit-identical on every route: COUNT, MIN / MAX (NaNs and the signs of zeros included), integer SUM / AVG"""
    if plan != "A" and tp != "i64":
        return ()
    return tuple(H.canon(v) for v in row)


ROW_PATH = _r("small")  # one dense key column, no LDS pre-aggregation, one push


@pytest.mark.parametrize("route,tp", CASES, ids=["%s-%s" % c for c in CASES])
def test_every_route_agrees_bit_for_bit_with_the_row_path(ctx, route, tp):
    """every route — those with key columns or a table of their own included — against the one-key row path over the SAME rows: every
    group, edge groups and fillers, has the same COUNT, MIN / MAX and integer SUM / AVG, bit for bit"""
    for plan in plans_for(route, tp):
        tbl = route_table(route, tp, designed(tp, plan))
        ref = run_route(ctx, ROW_PATH, tbl, plan)
        got = run_route(ctx, route, tbl, plan)
        assert set(got) == set(ref) and set(tbl.cells) <= set(ref)
        diff = [(k, tbl.names.get(k), ref[k], got[k]) for k in ref if _exact_image(tp, plan, got[k]) != _exact_image(tp, plan, ref[k])]
        assert not diff, (route, tp, plan, diff[:3])


# ---------------------------------------------------------------------------------------------------------------- the pinned rules
REAL_CASES = [c for c in CASES if c[1] in ("f64", "f32")]


@pytest.mark.parametrize("route,tp", REAL_CASES, ids=["%s-%s" % c for c in REAL_CASES])
def test_nan_ranks_by_its_sign_and_positive_zero_above_negative_zero(ctx, route, tp):
    """the device's rule for MIN / MAX of reals, exactly: the order of the memcomparable image (ord_image, tsq_agg.hip) —
    -NaN < -inf < .. < -0.0 < +0.0 < .. < +inf < +NaN, whatever the row order and on every route.  (The reference keeps whichever of a NaN and a number
    arrived first, and whichever zero: every answer below is one it can give.)"""
    g = dict(AE.EDGE_GROUPS[tp])
    pos_nan, neg_nan = AE.bits_of(AE.NAN, tp), AE.bits_of(g["neg_nan_alone"][0], tp)
    want = {  # group -> (MIN bits, MAX bits)
        "nan_between": (AE.bits_of(1.0, tp), pos_nan),
        "nan_first": (AE.bits_of(1.0, tp), pos_nan),
        "neg_nan_beside": (neg_nan, AE.bits_of(3.0, tp)),
        "neg_ones_nan_beside": (AE.bits_of(g["neg_ones_nan_alone"][0], tp), AE.bits_of(5.0, tp)),
        "pos_ones_nan_beside": (AE.bits_of(-1.0, tp), AE.bits_of(g["pos_ones_nan_alone"][0], tp)),
        "nan_and_infs": (AE.bits_of(-AE.INF, tp), pos_nan),
        "neg_then_pos_zero": (AE.bits_of(-0.0, tp), AE.bits_of(0.0, tp)),
        "pos_then_neg_zero": (AE.bits_of(-0.0, tp), AE.bits_of(0.0, tp)),
    }
    tbl = route_table(route, tp, designed(tp, "A"))
    rows = run_route(ctx, route, tbl, "A")
    seen = 0
    for k, name in tbl.names.items():
        if name in want:
            _, mn, mx = rows[k]
            assert (AE.bits_of(mn, tp), AE.bits_of(mx, tp)) == want[name], (name, mn, mx)
            seen += 1
    assert seen == len(want)
