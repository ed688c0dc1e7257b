"""CPU: tsq_eval_row / tsq_filter_row compiled with g++ (tests/hostsim) against the oracle on the edge-value grid of
tests/expr_edge.py, row by row, for every expression of all_exprs() and for the conjunct lists of the GPU filter tests.  This pins
the host build on the grid, so that a mismatch of tests/test_expr_edge_gpu.py which this file does not share is a finding about
the device compile (hipcc or hiprtc), not about the header."""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import expression as E
from tinysql_amd.chunk import make_cols

from . import expr_edge as X
from .test_hostsim_vs_oracle import all_exprs, sim, sim_eval  # noqa: F401  (sim: the module-scoped fixture)


def test_the_grid_is_the_one_the_gpu_tests_share(orc):
    g = X.grid()
    assert g.NumRows() == 441 and g.types() == X.TYPES and len(all_exprs()) == 75
    # row (a, b): NULLs exactly where the value lists say so
    for c, vals, of in ((0, X.IV, "a"), (1, X.IV, "b"), (2, X.UV, "a"), (3, X.UV, "b"), (4, X.FV, "a"), (5, X.FV, "b")):
        for r in range(441):
            a, b = divmod(r, 21)
            v = vals[a if of == "a" else b]
            assert g.columns[c].IsNull(r) == (v is None)
            if v is not None and c < 4:
                assert int(g.columns[c].data[r]) == v
            elif v is not None:
                assert np.float64(g.columns[c].data[r]).view(np.uint64) == np.float64(v).view(np.uint64)  # -0.0 stays -0.0
    total = sum(len(X.classify(orc, e).err) for e in all_exprs())
    fewest = min(len(X.classify(orc, e).ok) for e in all_exprs())
    print("oracle: %d (row, expression) pairs raise; fewest error-free rows per expression: %d" % (total, fewest))
    assert total > 2000 and fewest >= 150  # every expression keeps a large batch of rows whose VALUES are compared


@pytest.mark.parametrize("fam", X.FAMILIES)
def test_hostsim_equals_the_oracle_on_every_grid_row(sim, orc, fam):  # noqa: F811
    compared = raised = 0
    for i, e in X.exprs_of(fam):
        prog = E.compile_expr(e)
        assert sim.sim_validate(C.byref(prog), 7) == abi.OK
        want = X.classify(orc, e).per_row
        for r, one in enumerate(X.single_rows()):
            st, out, nn, w = sim_eval(sim, prog, one)
            if want[r][0] == "err":
                assert st == want[r][1], ("expression", i, "row", r)
                raised += 1
                continue
            assert st == abi.OK, ("expression", i, "row", r, st)
            assert (bool(nn[0]), w) == want[r][2:], ("NOT NULL flag / warnings", i, r)
            if want[r][2]:
                assert int(out[0]) == want[r][1], ("value bits", i, r, hex(int(out[0])), hex(want[r][1]))
            compared += 1
    assert compared > 0 and (raised > 0 or fam in ("compare", "rest"))


def sim_filter(sim, progs, n_progs, chk):  # noqa: F811
    keep = []
    cols = make_cols(chk.columns, keep)
    n = chk.NumRows()
    s, z, w = np.zeros(n, np.uint8), np.zeros(n, np.uint8), C.c_int64(0)
    st = sim.sim_filter_eval(progs, n_progs, cols, len(chk.columns), n, None, s.ctypes.data_as(C.c_void_p), z.ctypes.data_as(C.c_void_p), C.byref(w))
    return st, s.astype(bool), z.astype(bool), w.value


@pytest.mark.parametrize("kind", X.LIST_KINDS)
def test_hostsim_filter_equals_the_oracle_on_every_grid_row(sim, orc, kind):  # noqa: F811
    raised = 0
    lists = X.filter_lists(kind)
    assert len(lists) >= 8
    for i, lst in lists:
        progs = E.compile_list(lst)
        want = X.classify(orc, lst).per_row
        for r, one in enumerate(X.single_rows()):
            st, s, z, w = sim_filter(sim, progs, len(lst), one)
            if want[r][0] == "err":
                assert st == want[r][1], ("list of expression", i, "row", r)
                raised += 1
            else:
                assert (st, bool(s[0]), bool(z[0]), w) == (abi.OK,) + want[r][1:], ("list of expression", i, "row", r)
    assert raised > 0


def test_order_trees_fail_at_several_nodes_with_several_statuses(orc):
    """what the GPU first-error tests plant: every tree has rows failing at two nodes or more, with two statuses or more"""
    for name, tree, subs in X.order_trees():
        where = X.failing_nodes(orc, tree, subs)
        assert len({k for k, _ in where.values()}) >= 2 and len({s for _, s in where.values()}) >= 2, name
        assert len(X.classify(orc, tree).ok) >= 100, name
    _, tree, subs = X.order_trees()[3]
    at_first = {s for k, s in X.failing_nodes(orc, tree, subs).values() if k == 0}
    assert at_first == {abi.ERR_OVERFLOW_BIGINT, abi.ERR_OVERFLOW_BIGINT_UNSIGNED}  # one node, two statuses
