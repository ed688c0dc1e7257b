"""GPU: join keys at the edge values of tests/key_edge.py, on every route a join key can take through tsq_join.hip and its headers.

Key equality is codec.EqualChunkRow (util/codec/codec.go:212-240, 363-382: same flag, same 8 bytes); tsq_device.h tsq_key_word states it
once and every route restates it: ks.skip_high on the direct route, the 64-bit table words of the radix routes, the 32-byte key
records, the packed routes' `key - kmin` images, the LDS-build, LDS-dup and sorted-columns variants, the interval test, never_match.

Tables.  The build side holds every edge cell of its type once ("unique") or three times ("dup"), the probe side every edge cell of ITS
type twice; both hold NULL keys and ordinary filler keys up to the size a route needs (the probe side's fillers reach past the build
side's: some miss), and a payload column with the row number.  The expected joined rows come from the yardstick alone
(key_edge.join_pairs), as a multiset of bit patterns (H.multiset) with their number alongside; the oracle's join over the same
tables is compared with the yardstick as well, once per table.

The packed routes take integer keys whose build side lies in a narrow range: their build keys are a window of 8 192 keys at one of the
anchors [I64_MIN, ..), (.., I64_MAX], around -1 / 0, around 2^63 (U64), (.., U64_MAX], each probed with a column of its own
signedness and of the other; the probe side carries keys of the window, the cells just outside it on both sides (as 64-bit patterns:
below I64_MIN lies I64_MAX), and every edge cell of its type.

Every case names its route in a module-level table and asserts it from tsq_stats; a case that does not reach its route fails."""
import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column

from . import gpu_helpers as G
from . import helpers as H
from . import key_edge as KE

pytestmark = pytest.mark.gpu
FORCE, OFF = abi.RADIX_FORCE, abi.RADIX_OFF
INNER, LEFT = abi.JOIN_INNER, abi.JOIN_LEFT_OUTER

INT_PAIRS = [(b, p) for b in KE.INT_TYPES for p in KE.INT_TYPES]     # (build type, probe type)
REAL_PAIRS = [(b, p) for b in KE.REAL_TYPES for p in KE.REAL_TYPES]
MIXED_PAIRS = [("i64", "f64"), ("f64", "i64")]                         # flag 8 / 9 against flag 5: never_match, zero rows
SAME_CLASS = INT_PAIRS + REAL_PAIRS


# ---------------------------------------------------------------------------------------------------------------- tables
def _fillers(tp, lo, n):
    """ordinary keys, far from every edge cell (the reals are exact as float32)"""
    return [100_000 + lo + k for k in range(n)] if tp in KE.INT_TYPES else [100_000.5 + 0.25 * (lo + k) for k in range(n)]


class Sides:
    """the two key columns as cells, the chunks (key, row number), and the expected pairs of the yardstick"""

    def __init__(self, tpb, bcells, tpp, pcells, classes=None):
        self.tpb, self.tpp, self.bcells, self.pcells = tpb, tpp, bcells, pcells
        self.pairs = KE.join_pairs(tpb, bcells, tpp, pcells)
        self.classes = classes
        self.oracle_checked = set()

    def chunks(self, n_keys=1):
        def side(tp, cells, cls):
            extra = [Column(abi.I64, np.array(cls, dtype=np.int64))] if n_keys == 2 else []
            return Chunk([KE.column(tp, cells)] + extra + [Column(abi.I64, np.arange(len(cells), dtype=np.int64))])
        return side(self.tpb, self.bcells, self.classes[0] if self.classes else None), side(self.tpp, self.pcells, self.classes[1] if self.classes else None)

    def rows(self, jt, n_keys=1):
        """the joined rows (probe columns, then build columns) in probe order, build rows ascending: python cells"""
        cp = (lambda i: (self.classes[1][i],)) if n_keys == 2 else (lambda i: ())
        cb = (lambda j: (self.classes[0][j],)) if n_keys == 2 else (lambda j: ())
        out, at = [], 0
        for i, p in enumerate(self.pcells):
            hit = False
            while at < len(self.pairs) and self.pairs[at][0] == i:
                j = self.pairs[at][1]
                out.append((p,) + cp(i) + (i, self.bcells[j]) + cb(j) + (j,))
                at, hit = at + 1, True
            if not hit and jt == LEFT:
                out.append((p,) + cp(i) + (i,) + (None,) * (n_keys + 1))
        assert at == len(self.pairs)
        return out


_SIDES = {}


def grid_sides(tpb, tpp, dup, nb, npr):
    """edge cells + NULL keys + fillers, shuffled; classes: 0 an edge cell, 1 a filler, 2 a NULL key"""
    memo = (tpb, tpp, dup, nb, npr)
    if memo in _SIDES:
        return _SIDES[memo]
    rng = np.random.default_rng(nb * 7 + npr + 3 * KE.TYPE_NAMES.index(tpb) + KE.TYPE_NAMES.index(tpp) + (50 if dup else 0))
    be = KE.cells(tpb) * (3 if dup else 1)
    n_fill = nb - len(be) - 3
    if dup:  # about three rows per filler key
        keys = _fillers(tpb, 0, max(1, n_fill // 3))
        bf = [keys[i] for i in rng.integers(0, len(keys), n_fill)]
    else:
        bf = _fillers(tpb, 0, n_fill)
    bcells = be + [None] * 3 + bf
    bcls = [0] * len(be) + [2] * 3 + [1] * len(bf)
    pe = KE.cells(tpp) * 2
    span = max(1, n_fill // 3) if dup else n_fill
    pkeys = _fillers(tpp, -span // 8, span + span // 4)
    pf = [pkeys[i] for i in rng.integers(0, len(pkeys), npr - len(pe) - 5)]
    pcells = pe + [None] * 5 + pf
    pcls = [0] * len(pe) + [2] * 5 + [1] * len(pf)
    ob, op = rng.permutation(len(bcells)), rng.permutation(len(pcells))
    for tp, edge, fill in ((tpb, be, bf), (tpp, pe, pkeys)):  # no filler is an edge cell: "unique" is unique, a row's class is its key's
        assert not {KE.key_bits(tp, c) for c in edge} & {KE.key_bits(tp, c) for c in fill}
    s = Sides(tpb, [bcells[i] for i in ob], tpp, [pcells[i] for i in op], ([bcls[i] for i in ob], [pcls[i] for i in op]))
    if (tpb in KE.INT_TYPES) == (tpp in KE.INT_TYPES):
        assert len(s.pairs) > len(pf) // 2  # the fillers meet
    else:
        assert not s.pairs
    _SIDES[memo] = s
    return s


WINDOW = 8192
ANCHORS = {  # name -> (build type, the window's least key as a 64-bit pattern)
    "imin": ("i64", KE.I64_MIN & KE.M64),
    "imax": ("i64", KE.I64_MAX - WINDOW + 1),
    "zero": ("i64", (-WINDOW // 2) & KE.M64),
    "u63": ("u64", (1 << 63) - WINDOW // 2),
    "umax": ("u64", KE.U64_MAX - WINDOW + 1),
}
# (anchor, probe type).  Absent by design: ("imin", "u64") and ("umax", "i64") — across signedness only cells below 2^63 can match
# (codec.go:219-224), these windows hold none, and da_prepare leaves a build side without a usable row to the 64-bit routes
# (test_windows_without_a_usable_key_are_left_to_the_other_routes pins that, and their zero rows)
WINDOW_PAIRS = [("imin", "i64"), ("imax", "i64"), ("imax", "u64"), ("zero", "i64"), ("zero", "u64"), ("u63", "u64"), ("u63", "i64"), ("umax", "u64")]


def _cell(tp, w):
    w &= KE.M64
    return w - (1 << 64) if tp == "i64" and w >> 63 else w


def window_sides(anchor, tpp, kind, npr=20_000):
    """kind "unique": 6 000 keys of the window once; "dup": 2 000 keys three times; "full": every key once.  The window's first and
    last two keys and the three around its middle are always there."""
    memo = (anchor, tpp, kind, npr)
    if memo in _SIDES:
        return _SIDES[memo]
    tpb, kmin = ANCHORS[anchor]
    rng = np.random.default_rng(sum(map(ord, anchor + tpp + kind)))
    must = [0, 1, WINDOW // 2 - 1, WINDOW // 2, WINDOW // 2 + 1, WINDOW - 2, WINDOW - 1]
    rest = [int(d) for d in rng.permutation(WINDOW) if int(d) not in must]
    if kind == "full":
        offs = must + rest
    elif kind == "unique":
        offs = must + rest[:6000 - len(must)]
    else:
        offs = (must + rest[:2000 - len(must)]) * 3
    bcells = [_cell(tpb, kmin + d) for d in offs] + [None] * 3
    pe = KE.cells(tpp) * 2
    near = [_cell(tpp, kmin - d) for d in range(1, 40)] + [_cell(tpp, kmin + WINDOW - 1 + d) for d in range(1, 40)]
    inside = [_cell(tpp, kmin + int(d)) for d in rng.integers(0, WINDOW, npr - len(pe) - len(near) - 5)]
    pcells = pe + near + [None] * 5 + inside
    ob, op = rng.permutation(len(bcells)), rng.permutation(len(pcells))
    s = Sides(tpb, [bcells[i] for i in ob], tpp, [pcells[i] for i in op])
    assert len(s.pairs) > npr // 4 or (anchor, tpp) not in WINDOW_PAIRS
    _SIDES[memo] = s
    return s


# ---------------------------------------------------------------------------------------------------------------- running a case
def _check_oracle_once(orc, s, cfg, build, probe, jt, n_keys, count):
    """the oracle's join over the same tables against the yardstick: its rows, or their number for a COUNT(*) route"""
    if (jt, n_keys, count) in s.oracle_checked or (jt, n_keys, False) in s.oracle_checked:
        return
    want = orc.hash_join(cfg, build, probe)
    if count:
        assert want.NumRows() == len(s.pairs), "the oracle's join and the yardstick disagree"
    else:
        assert H.multiset(want) == H.multiset(s.rows(jt, n_keys)), "the oracle's join and the yardstick disagree"
    s.oracle_checked.add((jt, n_keys, count))


def run_case(ctx, orc, s, route):
    """one route over one pair of tables: the count or the rows against the yardstick, the statistics against the route"""
    r = ROUTES[route]
    n_keys = r.get("n_keys", 1)
    jt = r.get("jt", INNER)
    build, probe = s.chunks(n_keys)
    keys = list(range(n_keys))
    keep = []
    conds = [E.ScalarFunction("gt", E.ScalarFunction("plus", E.Column(n_keys, abi.I64), E.Column(2 * n_keys + 1, abi.I64)), E.Constant(-1))] if r.get("cond") else ()
    cfg = H.join_cfg(probe.types(), build.types(), keys, keys, jt, 1, conds, (), keep)
    count = r.get("count", False)
    assert not count or jt == INNER
    _check_oracle_once(orc, s, cfg, build, probe, jt, n_keys, count)
    stats = []
    with ctx.knobs(**r.get("knobs", {})):
        got = G.run_join(ctx, cfg, build, probe, chunk_rows=1 << 22, pull_rows=8192, count_only=count, radix=r.get("radix"),
                         packing=r.get("packing"), ordered=r.get("ordered"), stats_out=stats)
    r["check"](stats[0])
    if count:
        assert got == len(s.pairs), (route, got, len(s.pairs))
        return
    want_rows = s.rows(jt, n_keys)
    assert got.NumRows() == len(want_rows), (route, got.NumRows(), len(want_rows))
    if r.get("ordered"):  # MergeJoinExec's order: probe rows in order, each with its build rows in order
        assert [tuple(H.canon(v) for v in row) for row in got.rows()] == [tuple(H.canon(v) for v in row) for row in want_rows], route
    else:
        assert H.multiset(got) == H.multiset(want_rows), route


def _route_is(route, **more):
    def check(st):
        assert st.probe_route == route, (st.probe_route, route)
        for k, v in more.items():
            got = getattr(st, k)
            assert (got > 0) if v == "positive" else (got == v), (k, got, v)
    return check


NO_PACK = {"DA_MIN_BUILD_ROWS": 1 << 40}  # (keeps the integer shapes of the 64-bit routes away from the packed ones)
# route -> how it is forced (the way the route's own tests force it), what its statistics must say, which tables it runs on
ROUTES = {
    # 1. the direct route: the 64-bit table and ks.skip_high; never_match for the mixed-class pairs
    "direct_rows": dict(radix=OFF, packing=OFF, check=_route_is(abi.ROUTE_DIRECT, radix_batches=0), tables=("grid_dup", 400, 600), pairs=SAME_CLASS + MIXED_PAIRS),
    "direct_rows_left": dict(radix=OFF, packing=OFF, jt=LEFT, check=_route_is(abi.ROUTE_DIRECT, radix_batches=0), tables=("grid_dup", 400, 600), pairs=SAME_CLASS + MIXED_PAIRS),
    "direct_rows_unique": dict(radix=OFF, packing=OFF, check=_route_is(abi.ROUTE_DIRECT, radix_batches=0), tables=("grid_unique", 400, 600), pairs=SAME_CLASS + MIXED_PAIRS),
    "direct_count": dict(radix=OFF, packing=OFF, count=True, check=_route_is(abi.ROUTE_DIRECT, radix_batches=0), tables=("grid_dup", 400, 600), pairs=SAME_CLASS + MIXED_PAIRS),
    # 2. radix FORCE, COUNT(*): the L2 variant over a plain table, the LDS variant over a sliced one (32 768 build rows and more).
    # (never_match joins are not eligible: radix_eligible hands them to the direct route by design)
    "radix_l2_count": dict(radix=FORCE, packing=OFF, count=True, knobs={"RADIX_KERNEL_L2": 1}, check=_route_is(abi.ROUTE_RADIX_L2, radix_batches=1),
                           tables=("grid_dup", 3000, 6000), pairs=SAME_CLASS),
    "radix_lds_count": dict(radix=FORCE, packing=OFF, count=True, check=_route_is(abi.ROUTE_RADIX_LDS, radix_batches=1, table_slice_bits="positive"),
                            tables=("grid_dup", 33_000, 40_000), pairs=SAME_CLASS),
    "radix_lds_count_unique": dict(radix=FORCE, packing=OFF, count=True, check=_route_is(abi.ROUTE_RADIX_LDS, radix_batches=1, table_slice_bits="positive"),
                                   tables=("grid_unique", 33_000, 40_000), pairs=SAME_CLASS),
    # 3. key records: a second key column that copies the row class
    "keyrec_count": dict(radix=FORCE, n_keys=2, count=True, knobs=NO_PACK, check=_route_is(abi.ROUTE_KEYREC), tables=("grid_dup", 4000, 6000), pairs=SAME_CLASS),
    "keyrec_rows_cond": dict(radix=FORCE, n_keys=2, cond=True, knobs=NO_PACK, check=_route_is(abi.ROUTE_KEYREC), tables=("grid_dup", 4000, 6000), pairs=SAME_CLASS),
    "keyrec_rows_cond_left": dict(radix=FORCE, n_keys=2, cond=True, jt=LEFT, knobs=NO_PACK, check=_route_is(abi.ROUTE_KEYREC), tables=("grid_dup", 4000, 6000), pairs=SAME_CLASS),
    # 4. ordered output: rows in probe order
    "ordered": dict(ordered=True, check=_route_is(abi.ROUTE_DIRECT), tables=("grid_dup", 3000, 4000), pairs=SAME_CLASS + MIXED_PAIRS),
    "ordered_left": dict(ordered=True, jt=LEFT, check=_route_is(abi.ROUTE_DIRECT), tables=("grid_dup", 3000, 4000), pairs=SAME_CLASS + MIXED_PAIRS),
    # 5. the packed routes (integer pairs only: da_prepare refuses real keys by design, `!is_int_class(bt) || !is_int_class(pt)`)
    "packed_count_step": dict(radix=FORCE, packing=FORCE, count=True, knobs={"DA_INTERVAL": 0, "DA_PROBE_BITS": 0},
                              check=_route_is(abi.ROUTE_PACKED, packed_interval_batches=0, radix_batches=1), tables=("window", "dup"), pairs=WINDOW_PAIRS),
    "packed_count_bits": dict(radix=FORCE, packing=FORCE, count=True, knobs={"DA_INTERVAL": 0, "DA_PROBE_BITS": 4},
                              check=_route_is(abi.ROUTE_PACKED, packed_interval_batches=0, radix_batches=1), tables=("window", "unique"), pairs=WINDOW_PAIRS),
    "packed_count_interval": dict(radix=FORCE, packing=FORCE, count=True, knobs={"DA_INTERVAL": 2},
                                  check=_route_is(abi.ROUTE_PACKED, packed_interval_batches=1, radix_batches=1), tables=("window", "full"), pairs=WINDOW_PAIRS),
}
for _jt, _sfx in ((INNER, ""), (LEFT, "_left")):
    ROUTES["packed_lds_build1" + _sfx] = dict(radix=FORCE, packing=FORCE, jt=_jt, knobs={"DA_LDS_BUILD": 1},
                                              check=_route_is(abi.ROUTE_PACKED, packed_lds_bits="positive", packed_lds_dup=0), tables=("window", "unique"), pairs=WINDOW_PAIRS)
    ROUTES["packed_lds_build5" + _sfx] = dict(radix=FORCE, packing=FORCE, jt=_jt, knobs={"DA_LDS_BUILD": 5},
                                              check=_route_is(abi.ROUTE_PACKED, packed_lds_bits="positive", packed_lds_dup=0), tables=("window", "unique"), pairs=WINDOW_PAIRS)
    ROUTES["packed_lds_dup" + _sfx] = dict(radix=FORCE, packing=FORCE, jt=_jt, knobs={"DA_LDS_DUP": 2, "DA_LDS_BUILD": 1},
                                           check=_route_is(abi.ROUTE_PACKED, packed_lds_bits="positive", packed_lds_dup=1), tables=("window", "dup"), pairs=WINDOW_PAIRS)
    ROUTES["packed_sorted_cols" + _sfx] = dict(radix=FORCE, packing=FORCE, jt=_jt, knobs={"DA_LDS_BUILD": 0},
                                               check=_route_is(abi.ROUTE_PACKED, packed_lds_bits=0, packed_lds_dup=0), tables=("window", "unique"), pairs=WINDOW_PAIRS)
    ROUTES["packed_sorted_cols_dup" + _sfx] = dict(radix=FORCE, packing=FORCE, jt=_jt, knobs={"DA_LDS_BUILD": 0},
                                                   check=_route_is(abi.ROUTE_PACKED, packed_lds_bits=0, packed_lds_dup=0), tables=("window", "dup"), pairs=WINDOW_PAIRS)
CASES = [(route, a, b) for route, r in ROUTES.items() for a, b in r["pairs"]]


def sides_for(route, a, b):
    t = ROUTES[route]["tables"]
    if t[0] == "window":
        return window_sides(a, b, t[1])
    return grid_sides(a, b, t[0] == "grid_dup", t[1], t[2])


def test_route_table_is_complete():
    """printing CASES shows every (route, type pair | window, probe type) that runs; nothing is excluded at run time"""
    assert len(ROUTES) == 25 and len(CASES) == len(set(CASES))
    n = {route: len(r["pairs"]) for route, r in ROUTES.items()}
    assert all(n[r] == 10 for r in ("direct_rows", "direct_rows_left", "direct_rows_unique", "direct_count", "ordered", "ordered_left"))
    assert all(n[r] == 8 for r in ROUTES if r.startswith(("radix", "keyrec", "packed")))
    assert {a for a, _ in WINDOW_PAIRS} == set(ANCHORS) and all(ANCHORS[a][0] in KE.INT_TYPES and p in KE.INT_TYPES for a, p in WINDOW_PAIRS)


@pytest.mark.parametrize("route,a,b", CASES, ids=["%s-%s-%s" % c for c in CASES])
def test_edge_keys_on_every_route(ctx, orc, route, a, b):
    run_case(ctx, orc, sides_for(route, a, b), route)


@pytest.mark.parametrize("anchor,tpp", [("imin", "u64"), ("umax", "i64")])
def test_windows_without_a_usable_key_are_left_to_the_other_routes(ctx, orc, anchor, tpp):
    """a window of negative BIGINTs probed with BIGINT UNSIGNED cells, and the other way round: the same bytes, flag 8 against flag 9 —
    no row, and no packed images (da_prepare: `usable == 0`)"""
    s = window_sides(anchor, tpp, "unique")
    assert s.pairs == []
    build, probe = s.chunks()
    cfg = H.join_cfg(probe.types(), build.types(), [0], [0], INNER, 1)
    _check_oracle_once(orc, s, cfg, build, probe, INNER, 1, False)
    for count in (True, False):
        stats = []
        got = G.run_join(ctx, cfg, build, probe, chunk_rows=1 << 22, count_only=count, radix=FORCE, packing=FORCE, stats_out=stats)
        assert (got if count else got.NumRows()) == 0 and stats[0].probe_route != abi.ROUTE_PACKED
