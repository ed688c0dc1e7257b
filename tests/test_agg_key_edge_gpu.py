"""GPU: GROUP BY keys at the edge values of tests/key_edge.py, on every route a group key can take through tsq_agg.hip and its headers.

tests/test_agg_edge_gpu.py puts edge values into the ARGUMENT column and keeps the keys small integers; here the KEY column holds the
edge cells of one type — each between 1 and 5 times, NULL keys, filler groups up to the size at which a route engages — and the
argument is the row number.  The plan is FIRST_ROW(key), COUNT(*), SUM(arg), MIN(arg); the expected result is exactly the groups of
key_edge.groups_of (codec.HashGroupKey, util/codec/codec.go:713-746, float.go:22-30), each with its exact count, sum and minimum, and
a key whose bits are those of one of the group's own cells: either zero for the group of the zeros, a NaN's own bits for its group,
either cell for the group a NaN with the sign bit clear shares with a positive denormal (key_edge.agg_mismatch).  Fillers are checked
like the edge groups: the comparison is over the whole table.

The routes are those of tests/test_agg_edge_gpu.py (its ROUTES table is imported, with its sizes, knobs and statistics checks):
the row path, two key columns, L and H mode of the LDS pre-aggregation, the packed route with and without the dense state, the
partitioned groups, a string as second key column through the dictionary of group keys, six key columns through
tsq_agg_create_keys, the stream aggregate by lanes and in general — and their batch-splitting variants, in which the r-th row of every
group lies in half r mod 2 of the table (hash routes) or a batch boundary falls inside every group of two rows or more (stream
routes, whose rows arrive ordered by group: equal images adjacent, the edge groups in ascending order of their image).

The packed route takes integer keys of a narrow range only: its tables hold every key of a window of 5 000 keys at one of the anchors
[I64_MIN, ..), (.., I64_MAX], around -1 / 0, around 2^63 (U64) and (.., U64_MAX]; the window's first and last two keys and the three
around its middle are the edge cells."""
import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd.chunk import Chunk, Column, StrColumn, concat
from tinysql_amd.executor import AggFuncDesc, HashAggExec, MockDataSource

from . import gpu_helpers as G
from . import helpers as H
from . import key_edge as KE
from .test_agg_edge_gpu import GROUPS, HALF, ROUTES, STREAM_BATCH, _spread
from .test_agg_gpu import out_types_for

pytestmark = pytest.mark.gpu

WINDOW = 5000
ANCHORS = {  # name -> (key type, the window's least key)
    "imin": ("i64", KE.I64_MIN),
    "imax": ("i64", KE.I64_MAX - WINDOW + 1),
    "zero": ("i64", -WINDOW // 2),
    "u63": ("u64", (1 << 63) - WINDOW // 2),
    "umax": ("u64", KE.U64_MAX - WINDOW + 1),
}
PACKED = ("packed_dense", "packed_dense_split", "packed_no_dense_split")
# route of ROUTES -> the key types it runs with (absent: see the comment)
ALL = KE.TYPE_NAMES
ROUTE_TYPES = {
    "row": ALL, "row_split": ALL, "two_keys": ALL, "lds_l": ALL, "lds_l_split": ALL, "lds_h": ALL, "lds_h_split": ALL,
    "pg": ALL, "pg_split": ALL, "pg_small": ALL, "six_keys": ALL,
    "stream_lanes": ALL, "stream_lanes_split": ALL, "stream_general": ALL, "stream_general_split": ALL,
    # the dictionary of group keys takes integer and string key cells (tsq_agg.hip: `ok = t == TSQ_I64 || t == TSQ_U64 || t == TSQ_BYTES`):
    # a real first key beside a string goes the row path, which "two_keys" covers
    "str_key": KE.INT_TYPES,
    # the packed route takes integer keys (da_agg_setup): one case per window
    "packed_dense": KE.INT_TYPES, "packed_dense_split": KE.INT_TYPES, "packed_no_dense_split": KE.INT_TYPES,
    # packed_narrow16 / packed_narrow32 / packed_hot / packed_hot_off of ROUTES vary how the ARGUMENT cells travel and where a hot key's
    # rows are summed; the key's way through them is that of packed_dense_split
}
CASES = []
for _route, _types in ROUTE_TYPES.items():
    for _tp in _types:
        if _route in PACKED:
            CASES += [(_route, _tp, a) for a, (t, _) in ANCHORS.items() if t == _tp]
        else:
            CASES.append((_route, _tp, None))


def test_route_table_is_complete():
    """every route family of the issue is in the table, for every key type it accepts; nothing is excluded at run time"""
    assert set(ROUTE_TYPES) <= set(ROUTES)
    assert len(CASES) == 11 * 4 + 4 * 4 + 2 + 3 * 5 and len(set(CASES)) == len(CASES)
    assert {a for _, _, a in CASES if a} == set(ANCHORS)


# ---------------------------------------------------------------------------------------------------------------- tables
class KeyTable:
    """cells: the key cell of every row (None: NULL); the argument of row i is i; half: rows per device batch of the split variants;
    edge_images: the images of the edge groups (None: the NULL keys)"""

    def __init__(self, tp, cells, half, edge_images):
        self.tp, self.cells, self.half, self.edge_images = tp, cells, half, set(edge_images)
        self.args = list(range(len(cells)))
        self.images = [KE.group_image(tp, c) for c in cells]


def _filler_keys(tp, kind, n):
    if tp in KE.INT_TYPES:
        if kind == "spread":  # over 62 bits: no packed route
            return [int(v) for v in _spread(np.arange(1, n + 1))]
        return [1000 + k for k in range(n)]
    return [1000.5 + 0.25 * k for k in range(n)]  # (exact as float32)


def _edge_rows(tp, anchor, drop=()):
    """[(cell, copies)]: every edge cell 1 .. 5 times (but those named in `drop`)"""
    if anchor is None:
        cs = [c for n, c in KE.EDGE[tp] if n not in drop]
    else:
        kmin = ANCHORS[anchor][1]
        mid = kmin + WINDOW // 2
        cs = [kmin, kmin + 1, mid - 1, mid, mid + 1, kmin + WINDOW - 2, kmin + WINDOW - 1]
    return [(c, 1 + (i + len(drop)) % 5) for i, c in enumerate(cs)]


_TABLES = {}


def make_table(tp, size, kind, anchor=None, layout="alternate", drop=()):
    memo = (tp, size, kind, anchor, layout, drop)
    if memo in _TABLES:
        return _TABLES[memo]
    rng = np.random.default_rng(HALF[size] + 13 * KE.TYPE_NAMES.index(tp) + len(kind) + 7 * len(layout) + (sum(map(ord, anchor)) if anchor else 0))
    edge = _edge_rows(tp, anchor, drop)
    edge_images = {KE.group_image(tp, c) for c, _ in edge}
    if anchor is None:
        fill = _filler_keys(tp, kind, GROUPS[size] if layout != "straddle" else 2000)
    else:
        kmin = ANCHORS[anchor][1]
        fill = [kmin + k for k in range(WINDOW)]
    fill = [k for k in fill if KE.group_image(tp, k) not in edge_images]
    assert len(fill) >= (WINDOW - 7 if anchor else 30)
    if layout == "straddle":
        t = _straddle(rng, tp, edge, fill)
    else:
        half = HALF[size]
        halves, per_group = ([], []), {}
        for c, copies in edge + [(None, 3)]:
            img = KE.group_image(tp, c)
            for _ in range(copies):  # the r-th row of a GROUP in half r mod 2
                r = per_group.get(img, 0)
                per_group[img] = r + 1
                halves[r % 2].append(c)
        cells = []
        for h in (0, 1):
            part = halves[h] + [fill[i] for i in rng.integers(0, len(fill), half - len(halves[h]))]
            cells += [part[i] for i in rng.permutation(half)]
        t = KeyTable(tp, cells, half, edge_images | {None})
    assert not set(KE.groups_of(tp, [c for c, _ in edge])) - set(t.images)
    _TABLES[memo] = t
    return t


def _straddle(rng, tp, edge, fill):
    """rows in group order: the NULL keys, then the edge groups by ascending image, runs of filler groups between them so that a
    multiple of STREAM_BATCH falls inside every group of two rows or more (the group is open when a device batch ends)"""
    groups = {}
    for c, copies in edge + [(None, 3)]:
        groups.setdefault(KE.group_image(tp, c), []).extend([c] * copies)
    cells, next_fill = [], iter(fill)

    def fillers(n):
        while n > 0:
            run = min(n, int(rng.integers(1, 90)))
            cells.extend([next(next_fill)] * run)
            n -= run

    for img in sorted(groups, key=lambda i: (i is not None, i)):
        members = groups[img]
        members = [members[i] for i in rng.permutation(len(members))]  # (cells that share an image: mixed inside the group)
        if len(members) >= 2:
            fillers((-(len(cells) + (len(members) + 1) // 2)) % STREAM_BATCH)
        else:
            fillers(int(rng.integers(1, 40)))
        cells.extend(members)
    fillers(200)
    return KeyTable(tp, cells, STREAM_BATCH, set(groups))


def key_columns(kind, tbl):
    """the key columns of a route: the edge column first; the others are functions of the group, so the groups stay what they are"""
    first = KE.column(tbl.tp, tbl.cells)
    f = np.array([0 if i is None else i % 1009 for i in tbl.images], dtype=np.int64)
    if kind in ("dense", "spread"):
        return [first]
    if kind == "two":
        return [first, Column(abi.I64, f % 3 - 1)]
    if kind == "str":
        return [first, StrColumn([b"s%d" % (x % 5) for x in f.tolist()])]
    if kind == "six":
        return [first, Column(abi.I64, f % 7), Column(abi.I64, np.full(len(f), 3)), Column(abi.U64, (f % 2).astype(np.uint64)), Column(abi.I64, -f), Column(abi.I64, f * 5)]
    raise AssertionError(kind)


def run_route(ctx, route, tbl):
    """the rows (FIRST_ROW(key), COUNT(*), SUM(arg), MIN(arg)) of the table on the route"""
    r = ROUTES[route]
    key_cols = key_columns(r["keys"], tbl)
    nk = len(key_cols)
    chk = Chunk(key_cols + [Column(abi.I64, np.array(tbl.args, dtype=np.int64))])
    types = chk.types()
    aggs = [(abi.AGG_FIRSTROW, 0, types[0]), (abi.AGG_COUNT, -1, abi.I64), (abi.AGG_SUM, nk, abi.I64), (abi.AGG_MIN, nk, abi.I64)]
    if r["stream"]:  # equal images adjacent
        seen_done, last = set(), object()
        for img in tbl.images:
            if img != last:
                assert img not in seen_done, "the rows of a stream route are not ordered by group"
                seen_done.add(img)
                last = img
    if r["split"]:  # every group of two rows or more lies in two device batches
        for img, rows in KE.groups_of(tbl.tp, tbl.cells).items():
            if len(rows) >= 2 and img in tbl.edge_images:
                assert len({i // tbl.half for i in rows}) >= 2, (route, img)
    knobs = dict(r["knobs"])
    if r["split"]:
        knobs["AGG_BATCH_ROWS"] = tbl.half
    chunk_rows = tbl.half if r["split"] else 1 << 22
    stats = []
    with ctx.knobs(**knobs):
        if r["keys"] == "six":
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
    return got.rows()


def table_for(route, tp, anchor, drop=()):
    r = ROUTES[route]
    kind = "spread" if r["keys"] == "spread" else "dense"
    if r["stream"] and r["split"]:
        return make_table(tp, r["size"], kind, anchor, "straddle", drop)
    t = make_table(tp, r["size"], kind, anchor, drop=drop)
    if r["stream"]:  # a stable sort by image: NULL keys first, the rows of a group keep their shuffled order
        memo = (tp, r["size"], kind, anchor, "ordered", drop)
        if memo not in _TABLES:
            order = sorted(range(len(t.cells)), key=lambda i: (t.images[i] is not None, t.images[i] or 0))
            _TABLES[memo] = KeyTable(tp, [t.cells[i] for i in order], t.half, t.edge_images)
        t = _TABLES[memo]
    return t


@pytest.mark.parametrize("route,tp,anchor", CASES, ids=["%s-%s%s" % (r, t, "-" + a if a else "") for r, t, a in CASES])
def test_edge_keys_on_every_route(ctx, route, tp, anchor):
    tbl = table_for(route, tp, anchor)
    rows = run_route(ctx, route, tbl)
    wrong = KE.agg_mismatch(tp, tbl.cells, tbl.args, rows)
    assert wrong == "", "%s, %s keys%s: %s" % (route, tp, " at " + anchor if anchor else "", wrong)
    assert len(rows) == len(set(tbl.images)) > len(tbl.edge_images)


# the cells whose image another cell of the grid shares: without them a group's key can be one cell only
ALONE_DROP = ("+0", "nan_pos_ones", "denorm_7ffff")
REAL_ROUTES = [r for r, types in ROUTE_TYPES.items() if set(KE.REAL_TYPES) <= set(types)]


@pytest.mark.parametrize("tp", KE.REAL_TYPES)
@pytest.mark.parametrize("route", REAL_ROUTES)
def test_a_key_whose_image_is_not_invertible_comes_out_as_itself(ctx, route, tp):
    """the images of -0.0 and of a NaN with the sign bit clear are not invertible (key_edge.py): decodeCmpUintToFloat turns the first
    into +0.0 and the second into a positive denormal — for a float32 key, into 0.0.  The tables of test_edge_keys_on_every_route hold
    both zeros, and for float64 the denormal that shares the quiet NaN's image, so either cell is right there.  Pinned here, on every
    route that takes real keys: in a table WITHOUT +0.0, the all-ones NaN and that denormal, the group of -0.0 shows -0.0 and the
    groups of 0x7ff8000000000000 and 0x7ff8000000000001 (float32: 0x7fc00000, 0x7fc00001) show their own bits."""
    tbl = table_for(route, tp, None, ALONE_DROP)
    cells = dict(KE.EDGE[tp])
    assert not {KE.own_bits(tp, cells[n]) for n in ALONE_DROP if n in cells} & {KE.own_bits(tp, c) for c in tbl.cells if c is not None}
    rows = run_route(ctx, route, tbl)
    assert KE.agg_mismatch(tp, tbl.cells, tbl.args, rows) == ""
    for name in ("-0", "nan", "nan_p1"):
        want = KE.own_bits(tp, cells[name])
        members = {KE.own_bits(tp, tbl.cells[i]) for i in KE.groups_of(tp, tbl.cells)[KE.group_image(tp, cells[name])]}
        assert members == {want}, (name, members)  # (the group holds that cell alone, several times)
        keys = [r[0] for r in rows if r[0] is not None and KE.group_image(tp, r[0]) == KE.group_image(tp, cells[name])]
        assert len(keys) == 1 and KE.own_bits(tp, keys[0]) == want, (route, tp, name, keys)
