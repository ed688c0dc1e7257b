"""GPU: the joins' OtherConditions on the edge-value grid of tests/expr_edge.py, against the oracle's join.

The probe side carries the grid's left columns (I64, U64, F64 of value index a), the build side its right columns (I64, U64, F64
of value index b, and the F32 column); both carry the grid row number as the join key, so the join is one to one and its candidate
pairs are exactly the grid rows.  Every expression of all_exprs() is the join's condition once, taken as truthiness (toBool), on
the direct route (k_post_conds) and on the key-record route (k_kr_probe<.., COND>, forced by a second key column and
TSQ_RADIX_FORCE, asserted from the statistics), for inner and left outer joins.

On the pairs the oracle evaluates without an error the joined rows equal orc.hash_join's, cell by cell as bits; with one more pair
that raises, the join fails with the oracle's status (on the key-record route through its redo on the direct route)."""
import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd.chunk import Chunk, Column

from . import expr_edge as X
from . import gpu_helpers as G
from . import helpers as H

pytestmark = pytest.mark.gpu

ROUTES = ["direct", "keyrec"]
JOINS = [(abi.JOIN_INNER, "inner"), (abi.JOIN_LEFT_OUTER, "left_outer")]


def sides(idx, n_keys):
    """(probe, build) for the grid rows idx; n_keys key columns in front (the row number, and a copy of it)"""
    g = X.take(X.grid(), idx)
    keys = [Column(abi.I64, np.arange(len(idx), dtype=np.int64)) for _ in range(n_keys)]
    c = g.columns
    return Chunk(keys + [c[0], c[2], c[4]]), Chunk(keys + [c[1], c[3], c[5], c[6]])


def joined_index(n_keys):
    """grid column -> column of the joined row (probe columns, then build columns)"""
    p0, b0 = n_keys, n_keys + 3 + n_keys
    return {0: p0, 1: b0, 2: p0 + 1, 3: b0 + 1, 4: p0 + 2, 5: b0 + 2, 6: b0 + 3}


def remap(e, m):
    if isinstance(e, E.Column):
        return E.Column(m[e.index], e.tp)
    if isinstance(e, E.ScalarFunction):
        return E.ScalarFunction(e.name, *[remap(a, m) for a in e.args], no_unsigned_subtraction=e.force_signed)
    return e


def run(ctx, cfg, build, probe, route):
    stats = []
    got = G.run_join(ctx, cfg, build, probe, radix=abi.RADIX_FORCE if route == "keyrec" else abi.RADIX_OFF, stats_out=stats)
    return got, stats[0]


@pytest.mark.parametrize("jt,jt_name", JOINS, ids=[j[1] for j in JOINS])
@pytest.mark.parametrize("route", ROUTES)
@pytest.mark.parametrize("fam", X.FAMILIES)
def test_conditions_on_the_grid_pairs(ctx, orc, fam, route, jt, jt_name):
    n_keys = 2 if route == "keyrec" else 1
    want_route = abi.ROUTE_KEYREC if route == "keyrec" else abi.ROUTE_DIRECT
    m = joined_index(n_keys)
    key_idx = list(range(n_keys))
    failed = kept_some = 0
    for i, e in X.exprs_of(fam):
        cl = X.classify(orc, [e])  # the condition as a one-conjunct filter: which pairs raise, and what
        keep = []
        probe, build = sides(cl.ok, n_keys)
        cfg = H.join_cfg(probe.types(), build.types(), key_idx, key_idx, jt, 1, [remap(e, m)], (), keep)
        want = orc.hash_join(cfg, build, probe)
        got, st = run(ctx, cfg, build, probe, route)
        assert st.probe_route == want_route, ("expression", i, st.probe_route)
        passing = sum(1 for r in cl.ok if cl.per_row[r][1])
        assert want.NumRows() == (passing if jt == abi.JOIN_INNER else len(cl.ok)), ("the oracle's join and its filter disagree", i)
        assert got.NumRows() == want.NumRows() and H.multiset(got) == H.multiset(want), ("expression", i, got.NumRows(), want.NumRows())
        kept_some += 0 < passing < len(cl.ok)
        # one pair that raises, among the others
        for k, (status, row) in enumerate(sorted(cl.one_per_status().items())):
            idx, pos = X.with_row(cl.ok, row, i + k)
            probe, build = sides(idx, n_keys)
            with pytest.raises(orc.OracleError) as oe:
                orc.hash_join(cfg, build, probe)
            assert oe.value.status == status
            with pytest.raises(_lib.TsqError) as ge:
                run(ctx, cfg, build, probe, route)
            assert ge.value.status == status, ("expression", i, "grid row", row, "at", pos, ge.value.status, status)
            failed += 1
    assert kept_some > 0 and (failed > 0 or fam == "compare")
