"""GPU: the expression kernels on the edge-value grid of tests/expr_edge.py, against the oracle.

tsq_eval_row / tsq_filter_row reach the GPU through hipcc (the interpreter kernels k_expr_eval, k_filter_eval, the projection kernel
of tsq_project.h) and through hiprtc (jit_expr in its row layouts, jit_filter, jit_project); tests/test_expr_edge_cpu.py pins the
g++ build of the same header on the same grid.  Here every path sees the values at which an overflow check, a denormal, a signed
zero or a contracted multiply-add would show, and the first-error rule (atomicMin of tsq_errword over lanes and workgroups) is
exercised with errors in several workgroups at once.

No tolerances: data words, NOT NULL flags, selected / nulls flags are compared as bits, statuses and warning counts as integers.
The words of NULL results are not compared (a NULL slot of a result column holds no value: chunk.Column zeroes it on both sides)."""
import re

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import expression as E
from tinysql_amd import gpu_pipeline as GP
from tinysql_amd.chunk import Chunk, Column

from . import expr_edge as X
from .test_hostsim_vs_oracle import all_exprs
from .test_select_project_gpu import Project, oracle_chain, same

pytestmark = pytest.mark.gpu

# (id, jit mode, TSQ_KNOB_JIT_VARIANT or None for the default): the interpreter, and jit_expr in its default form, with one row
# slot of four rows per lane (0) and in the whole-wave coalesced layout (4)
PATHS = [("interp", abi.JIT_OFF, None), ("jit", abi.JIT_FORCE, None), ("jit_v0", abi.JIT_FORCE, 0), ("jit_v4", abi.JIT_FORCE, 4)]
PATH_IDS = [p[0] for p in PATHS]
JITS = [abi.JIT_OFF, abi.JIT_FORCE]
JIT_IDS = ["interp", "jit"]


def open_expr(ctx, exprs, path):
    """a handle on `path` (the variant knob is read when the handle's source is generated: set it first; the autouse fixture of
    conftest.py puts it back)"""
    _, jit, variant = path
    if variant is not None:
        ctx.set_knob(abi.KNOB_JIT_VARIANT, variant)
    return E.CompiledExpr(ctx, exprs, jit=jit)


def bits_of(col):
    nn = col.notnull if col.notnull is not None else np.ones(len(col), bool)
    return np.ascontiguousarray(col.data).view(np.uint64), nn


def eval_equals_oracle(ce, orc, prog, chk, what):
    want, ow = orc.expr_eval(prog, chk)
    w0 = ce.warnings
    got = ce.VecEval(chk)
    assert ce.warnings - w0 == ow, (what, "warnings", ce.warnings - w0, ow)
    (gd, gn), (wd, wn) = bits_of(got), bits_of(want)
    assert np.array_equal(gn, wn), (what, "NOT NULL flags differ at rows", np.nonzero(gn != wn)[0][:8])
    bad = np.nonzero(gd[wn] != wd[wn])[0]
    assert bad.size == 0, (what, "value bits differ", [(int(i), hex(int(gd[wn][i])), hex(int(wd[wn][i]))) for i in bad[:4]])


def raises_status(ce, chk):
    with pytest.raises(_lib.TsqError) as ei:
        ce.VecEval(chk)
    return ei.value.status


# ---------------------------------------------------------------- 3a. values
@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("part", list(X.EXPR_PARTS))
def test_values_on_the_error_free_rows(ctx, orc, part, path):
    g = X.grid()
    for i, e in X.EXPR_PARTS[part]:
        ok = X.classify(orc, e).ok
        prog = E.compile_expr(e)
        ce = open_expr(ctx, [e], path)
        try:
            eval_equals_oracle(ce, orc, prog, X.take(g, ok), ("expression", i, "error-free rows"))
            # 4133 rows: the bitmap words jit_expr writes itself and its ragged tail both carry edge rows
            eval_equals_oracle(ce, orc, prog, X.take(g, X.tiled(ok, X.BIG)), ("expression", i, "tiled"))
            # the whole grid behind a selection vector: the rows that would raise are there, and not selected
            eval_equals_oracle(ce, orc, prog, Chunk(g.columns, sel=ok.astype(np.int32)), ("expression", i, "selection vector"))
            if path[1] == abi.JIT_FORCE:
                assert ce.jit_launches() >= 3
        finally:
            ce.close()


# ---------------------------------------------------------------- 3b. every error row alone
@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("fam", X.FAMILIES)
def test_every_error_row_alone_raises_the_oracles_status(ctx, orc, fam, path):
    g = X.grid()
    k = launches = 0
    for i, e in X.exprs_of(fam):
        cl = X.classify(orc, e)
        if not cl.err:
            continue
        base = X.tiled(cl.ok, X.SMALL)
        ce = open_expr(ctx, [e], path)
        try:
            for row, status in cl.err:
                idx, pos = X.with_row(base, row, k)
                k += 1
                got = raises_status(ce, X.take(g, idx))
                assert got == status, ("expression", i, "grid row", row, "inserted at", pos, "status", got, "oracle", status)
                launches += 1
            if path[1] == abi.JIT_FORCE:
                assert ce.jit_launches() >= len(cl.err)
            # ... and the handle still evaluates: the error word of one call does not leak into the next
            eval_equals_oracle(ce, orc, E.compile_expr(e), X.take(g, base), ("expression", i, "after the errors"))
        finally:
            ce.close()
    print("%s/%s: %d error rows" % (fam, path[0], launches))
    assert launches > 0 or fam == "compare"  # (no comparison raises)


# ---------------------------------------------------------------- 3c. first-error order across workgroups
N_LAYOUTS = 24
LAST_WG = X.BIG - 256  # rows from here on belong to the last workgroups of a 256-lane launch
EDGES = [0, 1, 2, 3, 63, 64, 255, 256, 257, 1023, 1024, 2047, 2048, 4095, 4096, X.BIG - 1]


def layouts(orc, name, tree, subs):
    """[(description, {position in the 4133-row chunk: grid row})]: 2 to 6 planted rows failing at different nodes with different
    statuses; fixed seed.  The first layouts are the named ones of the issue, the rest random positions over edges and anywhere."""
    where = X.failing_nodes(orc, tree, subs)
    by_class = {}
    for r, ks in sorted(where.items()):
        by_class.setdefault(ks, []).append(r)
    classes = sorted(by_class)
    nodes = sorted({k for k, _ in classes})
    rng = np.random.default_rng(sum(map(ord, name)))
    pick = lambda ks: int(rng.choice(by_class[ks]))  # noqa: E731
    pairs = [(a, b) for a in classes for b in classes if a[0] < b[0] and a[1] != b[1]]
    early = pairs[0][0]                                      # the earliest node that has a later one with another status ...
    late = max(b for a, b in pairs if a == early)            # ... and the latest such node
    out = [("late node at row 0, early node in the last workgroup", {0: pick(late), int(rng.integers(LAST_WG, X.BIG)): pick(early)}),
           ("early node at row 0, late node in the last workgroup", {0: pick(early), int(rng.integers(LAST_WG, X.BIG)): pick(late)}),
           ("late node in the first wave, early node in the last row", {int(rng.integers(1, 64)): pick(late), X.BIG - 1: pick(early)}),
           ("late node in every workgroup, early node in the tail", dict([(256 * b + int(rng.integers(0, 256)), pick(late)) for b in range(5)]
                                                                          + [(X.BIG - 2, pick(early))]))]
    # one node, two statuses, two workgroups: the earlier ROW decides
    two = [n for n in nodes if len({s for k, s in classes if k == n}) >= 2]
    for n in two[:1]:
        a, b = [c for c in classes if c[0] == n][:2]
        p, q = int(rng.integers(0, 256)), int(rng.integers(LAST_WG, X.BIG))
        out.append(("one node, two statuses: %d first" % a[1], {p: pick(a), q: pick(b)}))
        out.append(("one node, two statuses: %d first" % b[1], {p: pick(b), q: pick(a)}))
        out.append(("one node, two statuses, a later node in front of both", {p + 256: pick(a), q: pick(b), 3: pick(max(classes))}
                    if max(classes)[0] > n else {p + 256: pick(b), q: pick(a)}))
    while len(out) < N_LAYOUTS:
        m = int(rng.integers(2, 7))
        chosen = [classes[j] for j in rng.permutation(len(classes))[:m]]
        while len(chosen) < m:
            chosen.append(classes[int(rng.integers(len(classes)))])
        if len({k for k, _ in chosen}) < 2 or len({s for _, s in chosen}) < 2:
            continue
        pos = set()
        while len(pos) < m:
            pos.add(int(rng.choice(EDGES)) if rng.random() < 0.5 else int(rng.integers(0, X.BIG)))
        out.append(("random %d" % len(out), dict(zip(sorted(pos, key=lambda _: rng.random()), [pick(c) for c in chosen]))))
    return out


_order_cases = {}


def order_case(orc, t):
    """(tree, [(description, chunk, the oracle's status for the whole chunk)], how many of the chunks tell the rule from "the first
    ROW wins"): computed once, shared by the four paths"""
    if t not in _order_cases:
        name, tree, subs = X.order_trees()[t]
        where = X.failing_nodes(orc, tree, subs)
        telling = 0
        prog = E.compile_expr(tree)
        g = X.grid()
        base = X.tiled(X.classify(orc, tree).ok, X.BIG)
        cases = []
        for what, planted in layouts(orc, name, tree, subs):
            idx = base.copy()
            for pos, row in planted.items():
                idx[pos] = row
            chk = X.take(g, idx)
            with pytest.raises(orc.OracleError) as oe:
                orc.expr_eval(prog, chk)
            cases.append((what, chk, oe.value.status))
            telling += where[planted[min(planted)]][1] != oe.value.status
        _order_cases[t] = (tree, cases, telling)
    return _order_cases[t]


@pytest.mark.parametrize("path", PATHS, ids=PATH_IDS)
@pytest.mark.parametrize("t", range(4), ids=[t[0] for t in X.order_trees()])
def test_first_error_is_first_node_then_first_row_across_workgroups(ctx, orc, t, path):
    tree, cases, telling = order_case(orc, t)
    assert len(cases) >= 20 and telling >= 5  # (an evaluator that ordered errors by row alone would miss `telling` of them)
    ce = open_expr(ctx, [tree], path)
    try:
        for what, chk, status in cases:
            got = raises_status(ce, chk)
            print("%-62s status %d oracle %d" % (what, got, status))
            assert got == status, (what, got, status)
        if path[1] == abi.JIT_FORCE:
            assert ce.jit_launches() >= len(cases)
    finally:
        ce.close()


# ---------------------------------------------------------------- 4a. VectorizedFilter
@pytest.mark.parametrize("jit", JITS, ids=JIT_IDS)
@pytest.mark.parametrize("part", list(X.LIST_PARTS))
def test_filter_lists_on_the_grid(ctx, orc, part, jit):
    g = X.grid()
    planted = 0
    for i, lst in X.LIST_PARTS[part]:
        cl = X.classify(orc, lst)
        ce = E.CompiledExpr(ctx, lst, jit=jit)
        try:
            for what, chk in (("error-free rows", X.take(g, cl.ok)), ("tiled", X.take(g, X.tiled(cl.ok, X.BIG))),
                              ("selection vector", Chunk(g.columns, sel=cl.ok.astype(np.int32)))):
                osel, onull, ow = orc.filter_eval(ce.progs, len(lst), chk)
                w0 = ce.warnings
                sel, nulls = ce.VectorizedFilter(chk, want_nulls=True)
                assert np.array_equal(sel, osel), ("list of expression", i, what, "selected differs at", np.nonzero(sel != osel)[0][:8])
                assert np.array_equal(nulls, onull), ("list of expression", i, what, "nulls differ at", np.nonzero(nulls != onull)[0][:8])
                assert ce.warnings - w0 == ow, ("list of expression", i, what, "warnings", ce.warnings - w0, ow)
            base = X.tiled(cl.ok, X.SMALL)
            for status, row in sorted(cl.one_per_status().items()):
                idx, pos = X.with_row(base, row, planted)
                planted += 1
                with pytest.raises(_lib.TsqError) as ei:
                    ce.VectorizedFilter(X.take(g, idx), want_nulls=True)
                assert ei.value.status == status, ("list of expression", i, "grid row", row, "at", pos, ei.value.status, status)
            if jit == abi.JIT_FORCE:
                assert ce.jit_launches() >= 3
        finally:
            ce.close()
    assert planted > 0


# ---------------------------------------------------------------- 4b. the fused Selection + Projection operator
GROUP = 16
N_GROUPS = (75 + GROUP - 1) // GROUP
KEEP = E.Column(7, abi.I64)  # an eighth column: the filter eq(c7, 1) selects exactly the rows the case wants


def with_flag(chk, flags):
    return Chunk(chk.columns + [Column(abi.I64, np.asarray(flags, np.int64))])


@pytest.mark.parametrize("jit", JITS, ids=JIT_IDS)
@pytest.mark.parametrize("grp", range(N_GROUPS))
def test_project_groups_of_sixteen_outputs(ctx, orc, grp, jit):
    exprs = all_exprs()
    assert len(exprs) == 75
    outs = exprs[grp * GROUP:(grp + 1) * GROUP]
    cls = [X.classify(orc, e) for e in outs]
    bad = np.zeros(X.NROWS, bool)
    for cl in cls:
        bad[[r for r, _ in cl.err]] = True
    assert (~bad).sum() >= 50  # (the three int operators over four sign combinations share 57 error-free rows, the other groups more)
    filt = [X.F("eq", KEEP, X.K(1))]
    g = X.grid()
    dev_chunks = []
    p = Project(ctx, filt, outs, jit)
    try:
        def run(chk):
            dev = GP.DeviceChunk.from_host(ctx, chk)
            dev_chunks.append(dev)
            return p.run(dev)
        # the filter deselects exactly the union of the group's error rows
        chk = with_flag(g, ~bad)
        want = oracle_chain(chk, filt, outs)
        assert want[0] == abi.OK and want[1] == int((~bad).sum())
        same(run(chk), want)
        # the same 4133 rows long: error rows in every workgroup, none selected
        idx = X.tiled(np.arange(X.NROWS), X.BIG)
        big = with_flag(X.take(g, idx), ~bad[idx])
        want = oracle_chain(big, filt, outs)
        assert want[0] == abi.OK
        same(run(big), want)
        # one error row let through: the first failing output decides.  One row per (first failing output, status)
        seen = set()
        for r in np.nonzero(bad)[0]:
            first = next((j, cl.per_row[r][1]) for j, cl in enumerate(cls) if cl.per_row[r][0] == "err")
            if first in seen:
                continue
            seen.add(first)
            flags = ~bad
            flags[r] = True
            chk = with_flag(g, flags)
            want = oracle_chain(chk, filt, outs)
            assert want[0] == first[1]
            got = run(chk)
            assert got[0] == want[0], ("grid row", int(r), "first failing output", first[0], "status", got[0], "oracle", want[0])
            assert re.search(r"output %d\b" % first[0], p.message()), p.message()
        ev, jl, _ = p.stats()
        assert ev == 2 + len(seen) and (jit != abi.JIT_FORCE or jl == ev), (ev, jl, p.message())
    finally:
        p.close()
        for d in dev_chunks:
            d.free()
