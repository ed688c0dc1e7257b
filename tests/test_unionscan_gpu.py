"""GPU parity of tsq_unionscan_* (UnionScanExec, executor/union_scan.go:89-300) with tests/unionscan_ref.py, the plain Python
restatement of getSnapshotRow / getOneRow / compare.  Every case is also checked the second way (kept snapshot rows + added rows
sorted by (keys, handle): Case.want).  Rows are compared exactly, cell for cell — NULL flags, string bytes, the bits of reals."""
import ctypes as C
import random

import numpy as np
import pytest

from tests import unionscan_cases as UC
from tests.unionscan_ref import UnionScanRef, canon, chunk_of
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import executor as X
from tinysql_amd import gpu_pipeline as P
from tinysql_amd.chunk import chunk_from_buffers, make_cols, out_buffers

pytestmark = pytest.mark.gpu


def dirty_of(cs):
    d = X.DirtyTable()
    d.addedRows, d.deletedRows = set(cs.added_handles), set(cs.deleted_handles)
    return d


class Handle:
    """one tsq_unionscan through the C-ABI, host columns"""

    def __init__(self, ctx, cs, cap=1024):
        self.ctx, self.lib, self.cs, self.cap = ctx, ctx.lib, cs, cap
        self.h = X.unionscan_create(ctx, X.unionscan_cfg(cs.types, cs.used_index, cs.handle_idx, cs.desc, cap), dirty_of(cs))

    def call(self, name, rows):
        chk, keep = chunk_of(self.cs.types, rows), []
        return getattr(self.lib, name)(self.h, make_cols(chk.columns, keep), len(chk.columns), len(rows))

    def set_added(self, rows=None):
        _lib.check(self.call("tsq_unionscan_set_added", self.cs.added_rows if rows is None else rows), self.h)

    def push(self, rows):
        _lib.check(self.call("tsq_unionscan_push", rows), self.h)

    def finish(self):
        _lib.check(self.lib.tsq_unionscan_finish(self.h), self.h)

    def pull(self, cap=None):
        """(rows, eos) of one pull; the peek before it must announce exactly what the pull writes"""
        types, cap, keep = self.cs.types, cap or self.cap, []
        nc = len(types)
        vb, pn = (C.c_int64 * nc)(), C.c_int64(0)
        _lib.check(self.lib.tsq_unionscan_peek(self.h, cap, C.byref(pn), vb, nc), self.h)
        out, bufs = out_buffers(types, cap, keep, list(vb))
        n, eos = C.c_int64(0), C.c_int32(0)
        _lib.check(self.lib.tsq_unionscan_pull(self.h, out, nc, cap, C.byref(n), C.byref(eos)), self.h)
        assert pn.value == n.value <= cap
        for c, tp in enumerate(types):
            assert vb[c] == (int(bufs[c][2][n.value]) if tp == abi.BYTES and n.value else 0)
            if tp == abi.BYTES and n.value:
                assert bufs[c][2][0] == 0 and (np.diff(bufs[c][2][:n.value + 1]) >= 0).all()
        return chunk_from_buffers(types, bufs, n.value).rows(), eos.value

    def pull_all(self):
        rows = []
        while True:
            r, eos = self.pull()
            rows += r
            if not r:
                return rows, eos

    def stats(self):
        a, b, c, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_unionscan_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(ms)), self.h)
        return a.value, b.value, c.value, ms.value

    def close(self):
        if self.h:
            self.lib.tsq_unionscan_destroy(self.h)
            self.h = None


def run_abi(ctx, cs, cuts=(), check_prefix=False, cap=1024):
    """the case through the C-ABI, the snapshot rows cut into pushes; with check_prefix everything is pulled after every push and the
    count is checked against the streaming rule computed in Python"""
    u = Handle(ctx, cs, cap)
    try:
        u.set_added()
        got, kept = [], []
        for chunk in cs.cut(cuts):
            u.push(chunk)
            if check_prefix:
                rows, eos = u.pull_all()
                assert eos == 0
                got += rows
                kept += cs.ref.keep(chunk)
                assert len(got) == cs.ref.determined(kept), (cs.name, len(kept))
        u.finish()
        rows, eos = u.pull_all()
        assert eos == 1
        assert u.pull() == ([], 1)
        st = u.stats()
        n_kept = len(cs.ref.keep(cs.snapshot))
        assert st[:3] == (len(cs.snapshot), len(cs.snapshot) - n_kept, len(cs.added_rows)), cs.name
        return got + rows
    finally:
        u.close()


def same(cs, got, want=None):
    want = cs.want() if want is None else want
    assert len(got) == len(want), cs.name
    assert canon(cs.types, got) == canon(cs.types, want), cs.name


class ListSource(P.GpuExecutor):
    """device chunks of host rows, one per Next"""

    def __init__(self, ctx, types, chunks):
        super().__init__(ctx, types)
        self.host, self.live, self.at = [chunk_of(types, c) for c in chunks if c], [], 0

    def Open(self):
        self.at = 0

    def Next(self):
        if self.at >= len(self.host):
            return P.EOS
        self.live.append(P.DeviceChunk.from_host(self.ctx, self.host[self.at]))
        self.at += 1
        return self.live[-1]

    def Close(self):
        for c in self.live:
            c.free()
        self.live = []


def run_executor(ctx, cs, chunk_rows=1024, conditions=None, added=None):
    src = X.MockDataSource(ctx, chunk_of(cs.types, cs.snapshot), chunk_rows)
    exe = X.UnionScanExec(ctx, src, dirty_of(cs), chunk_of(cs.types, cs.added_rows if added is None else added), cs.used_index, cs.handle_idx, cs.desc,
                          conditions=conditions, max_chunk_size=chunk_rows)
    return [r for c in X.drain(exe) for r in c.rows()]


def run_pipeline(ctx, cs, cuts=(), pull_rows=1 << 12, conditions=None, added=None):
    exe = P.GpuUnionScanExec(ctx, ListSource(ctx, cs.types, cs.cut(cuts)), dirty_of(cs), chunk_of(cs.types, cs.added_rows if added is None else added),
                             cs.used_index, cs.handle_idx, cs.desc, conditions=conditions, pull_rows=pull_rows)
    return [r for c in P.drain_device(exe) for r in c.rows()]


# ---------------------------------------------------------------- the reference's own rows
@pytest.mark.parametrize("i", range(len(UC.GOLDEN)))
def test_rows_of_TestDirtyTransaction_through_every_layer(ctx, i):
    steps, used, desc, want = UC.GOLDEN[i]
    cs = UC.txn_case(UC.SNAP, steps, used, desc)
    assert run_abi(ctx, cs) == want
    assert run_abi(ctx, cs, cuts=[1, 1], check_prefix=True) == want
    assert run_executor(ctx, cs, 2) == want
    assert run_pipeline(ctx, cs, cuts=[2]) == want


def test_delete_all_then_insert_and_the_unsigned_pk_rows(ctx):
    snap = [(1, 1), (2, 2)]  # union_scan_test.go:75-79
    assert run_abi(ctx, UC.txn_case(snap, [("delete", [1, 2])], [], False)) == []
    for used in ([], [1]):
        cs = UC.txn_case(snap, [("delete", [1, 2]), ("insert", [(3, 1)])], used, False)
        assert run_abi(ctx, cs) == [(3, 1)] and run_pipeline(ctx, cs) == [(3, 1)] and run_executor(ctx, cs) == [(3, 1)]
    types = [abi.U64, abi.I64, abi.BYTES]  # :92-98: an added handle (0) whose row the reader's condition filtered out
    cs = UC.Case(types, 0, [1, 0, 2], False, [], [(1, 1, None)], [0, 1], [])
    assert run_abi(ctx, cs) == [(1, 1, None)]
    cs = UC.Case(types, 0, [1, 0, 2], False, [], [(3, 3, b"a")], [0, 1, 2, 3], [])
    assert run_abi(ctx, cs) == [(3, 3, b"a")] and run_pipeline(ctx, cs) == [(3, 3, b"a")]


def test_conditions_filter_the_added_rows_in_both_executors(ctx):
    from tinysql_amd import expression as E
    cs = UC.txn_case(UC.SNAP, [UC.INS], [], False)
    cond = [E.ScalarFunction("gt", E.Column(1, abi.I64), E.Constant(4))]  # b > 4 on the added rows: (3, 4) goes, its handle stays dirty
    all_added = cs.added_rows
    kept = [r for r in all_added if r[1] > 4]
    want = UnionScanRef(cs.types, cs.added_handles, [], kept, [], 0, False).run([cs.snapshot])
    assert want == [(1, 5), (2, 3), (4, 8), (6, 8), (7, 6)]
    assert run_executor(ctx, cs, conditions=cond) == want
    assert run_pipeline(ctx, cs, conditions=cond) == want


# ---------------------------------------------------------------- tile edges
@pytest.mark.parametrize("kind", UC.INTERLEAVINGS)
def test_tile_edges(ctx, kind):
    for total in UC.TILE_TOTALS:
        cs = UC.table_case(kind, total)
        same(cs, run_abi(ctx, cs))
    for total in (65, 4097):
        cs = UC.table_case(kind, total, desc=True)
        same(cs, run_abi(ctx, cs, cuts=[total // 3]))


# ---------------------------------------------------------------- push shapes
def shape_case():
    cs = UC.table_case("runs_1000", 4097)
    drop = [r[0] for r in cs.snapshot[1000:1010]] + [r[0] for r in cs.snapshot[40:1000:7]]  # rows 1000..1009: a 1-row push (and a 10-row one) loses everything
    return UC.Case(cs.types, 0, [], False, cs.snapshot, cs.added_rows, cs.added_handles, drop, "shapes")


@pytest.fixture(scope="module")
def shape():
    cs = shape_case()
    return cs, cs.want()


@pytest.mark.parametrize("how", ["one", "rows_1", "rows_1024", "random", "all_dropped_push"])
def test_push_shapes_give_the_same_sequence(ctx, shape, how):
    cs, want = shape
    n = len(cs.snapshot)
    if how == "one":
        cuts = []
    elif how == "rows_1":
        cuts = [1] * n
    elif how == "rows_1024":
        cuts = [1024] * (n // 1024)
    elif how == "random":
        rng, cuts = random.Random(9), []
        while sum(cuts) < n:
            cuts.append(rng.choice([1, 2, 7, 64, 500, 1500]))
    else:
        cuts = [1000, 10, 300]  # the second push holds deleted rows only
        assert cs.ref.keep(cs.snapshot[1000:1010]) == []
    same(cs, run_abi(ctx, cs, cuts=cuts, check_prefix=True), want)
    if how in ("one", "rows_1024", "all_dropped_push"):
        same(cs, run_pipeline(ctx, cs, cuts=cuts, pull_rows=1000), want)


# ---------------------------------------------------------------- handles
@pytest.mark.parametrize("desc", [False, True])
def test_edge_handles_and_the_unsigned_handle_column(ctx, desc):
    for tp in (abi.I64, abi.U64):
        for which in (0, 1):
            cs = UC.edge_handle_case(tp, desc, which)
            got = run_abi(ctx, cs, cuts=[2], check_prefix=True)
            same(cs, got)
            if tp == abi.U64 and which == 0 and not desc:  # 0x8000000000000000 read through TSQ_U64 sorts as INT64_MIN: first
                assert got[0][0] == 1 << 63 and got[-1][0] == (1 << 63) - 2


def test_handles_that_collide_modulo_the_table_size(ctx):
    cs = UC.colliding_case()
    assert ctx.lib.tsq_unionscan_set_slots(len(cs.deleted_handles)) == 128
    same(cs, run_abi(ctx, cs, cuts=[17, 30]))


@pytest.fixture(scope="module")
def big():
    """2^20 snapshot rows (BIGINT handle, BIGINT, DOUBLE) in table order, as columns and as row tuples"""
    n = 1 << 20
    h = np.arange(n, dtype=np.int64) * 3 - (n // 2)
    rows = list(zip(h.tolist(), (h % 7 - 3).tolist(), (h * 0.5).tolist()))
    return h, rows


@pytest.mark.parametrize("n_set", [0, 1, 1000, 1 << 20])
def test_set_sizes_over_2p20_snapshot_rows(ctx, big, n_set):
    h, rows = big
    n = len(h)
    rng = np.random.default_rng(n_set)
    n_added = min(n_set // 2, 1000)  # added handles, each with a row that falls between two snapshot handles
    added_h = np.sort(rng.choice(n, n_added, replace=False).astype(np.int64) * 3 - (n // 2) + 1)
    n_del = n_set - n_added
    hit = rng.choice(n, min(n_del, n // 2), replace=False)  # deleted handles that snapshot rows have ...
    deleted = h[hit].tolist() + list(range(1 << 40, (1 << 40) + n_del - len(hit)))  # ... and deleted handles no row has
    cs = UC.Case(UC.T3, 0, [], False, rows, [UC.row3(int(x)) for x in added_h], added_h.tolist(), deleted, "set-%d" % n_set)
    assert len(cs.added_handles) + len(cs.deleted_handles) == n_set
    got = run_abi(ctx, cs, cuts=[1 << 18, 1 << 19], cap=1 << 20)
    assert got == cs.ref.run([cs.snapshot])
    keep = np.ones(n, bool)
    keep[hit] = False
    second = np.sort(np.concatenate([h[keep], added_h]))  # the second way, in numpy
    assert [r[0] for r in got] == second.tolist()


def test_an_added_handle_without_a_row_drops_the_snapshot_row(ctx):
    cs = UC.Case(UC.T3, 0, [], False, [UC.row3(h) for h in (1, 2, 3, 4)], [UC.row3(10)], [3, 10], [])
    assert [r[0] for r in run_abi(ctx, cs)] == [1, 2, 4, 10]


# ---------------------------------------------------------------- keys and payload
@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("tp", [abi.I64, abi.U64, abi.F32, abi.F64, abi.BYTES])
def test_one_key_of_each_type(ctx, tp, desc):
    cs = UC.one_key_case(tp, desc)
    want = cs.want()
    nulls = [r[1] is None for r in want]
    assert any(nulls) and (all(nulls[-nulls.count(True):]) if desc else all(nulls[:nulls.count(True)]))  # NULL first ascending, last under desc
    same(cs, run_abi(ctx, cs, cuts=[100, 1, 50], check_prefix=True), want)
    same(cs, run_pipeline(ctx, cs, cuts=[64]), want)


@pytest.mark.parametrize("desc", [False, True])
@pytest.mark.parametrize("n_keys", [2, 4])
def test_mixed_keys(ctx, n_keys, desc):
    cs = UC.multi_key_case(n_keys, desc)
    want = cs.want()
    same(cs, run_abi(ctx, cs, cuts=[77, 200], check_prefix=True), want)
    same(cs, run_executor(ctx, cs, 128), want)


@pytest.mark.parametrize("desc", [False, True])
def test_sixteen_columns_with_nullable_and_var_len_payload(ctx, desc):
    cs = UC.payload_case(desc)
    want = cs.want()
    same(cs, run_abi(ctx, cs, cuts=[300], cap=100), want)
    same(cs, run_pipeline(ctx, cs, cuts=[9, 300], pull_rows=64), want)
    same(cs, run_executor(ctx, cs, 50), want)


# ---------------------------------------------------------------- protocol
def test_wrong_call_order_and_cancel(ctx):
    cs = UC.txn_case(UC.SNAP, [UC.INS], [], False)
    u = Handle(ctx, cs)
    try:
        assert u.pull() == ([], 0)  # nothing pushed yet: more input is needed
        u.set_added()
        assert u.call("tsq_unionscan_set_added", cs.added_rows) == abi.ERR_INVALID and "already" in _lib.last_error(u.h)
        u.push(cs.snapshot[:1])
        assert u.call("tsq_unionscan_set_added", cs.added_rows) == abi.ERR_INVALID
        u.finish()
        assert u.call("tsq_unionscan_push", cs.snapshot[1:]) == abi.ERR_INVALID and "after finish" in _lib.last_error(u.h)
        u.finish()  # idempotent
        assert u.pull_all()[0] == [(1, 5), (2, 3), (3, 4), (7, 6)]
    finally:
        u.close()
    u = Handle(ctx, cs)
    try:
        assert u.call("tsq_unionscan_push", cs.snapshot) == abi.OK
        assert u.call("tsq_unionscan_set_added", cs.added_rows) == abi.ERR_INVALID and "after a push" in _lib.last_error(u.h)
        assert ctx.lib.tsq_unionscan_cancel(u.h) == abi.OK
        n, eos = C.c_int64(0), C.c_int32(0)
        assert u.call("tsq_unionscan_push", cs.snapshot) == abi.ERR_CANCELLED
        assert ctx.lib.tsq_unionscan_finish(u.h) == abi.ERR_CANCELLED
        assert ctx.lib.tsq_unionscan_pull(u.h, None, 2, 10, C.byref(n), C.byref(eos)) == abi.ERR_CANCELLED
    finally:
        u.close()
    bad = X.unionscan_cfg([abi.I64, abi.F64], [], 1, False, 1024)  # the handle column must be an 8-byte integer column
    h = C.c_void_p()
    assert ctx.lib.tsq_unionscan_create(ctx.h, C.byref(bad), None, 0, None, 0, C.byref(h)) == abi.ERR_INVALID
