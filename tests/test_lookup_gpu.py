"""GPU parity of tsq_lookup_* (the table worker of IndexLookUpExecutor, executor/distsql.go:558-637) with tests/lookup_ref.py, the
numpy restatement.  Row ordinals and handles are compared exactly, in emission order."""
import ctypes as C

import numpy as np
import pytest

from tests import lookup_ref as LR
from tinysql_amd import _abi as abi
from tinysql_amd import _lib

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
GUARD = 16  # int64 words on each side of an output
PATTERN = 0x5A5A5A5A5A5A5A5A
TABLE_SIZES = [0, 1, 2, 63, 64, 65, 255, 256, 257, 4097, 70001]
TASK_SIZES = [0, 1, 63, 64, 65, 2049, 50000]
STRIDES = [0, 2, 6, None]  # TSQ_KNOB_LOOKUP_STRIDE; None = the default


def make_table(n, seed=1):
    """n strictly ascending handles: both int64 extremes, runs of consecutive values, gaps"""
    if n == 0:
        return np.zeros(0, np.int64)
    rng = np.random.default_rng(seed + n)
    gaps = rng.integers(2, 1 << 36, n).astype(np.int64)
    gaps[rng.random(n) < 0.5] = 1
    t = -(1 << 48) + np.cumsum(gaps)
    t[-1] = I64_MAX
    if n >= 2:
        t[0] = I64_MIN
    return t.astype(np.int64)


_TABLES = {}


def table_of(n):
    if n not in _TABLES:
        _TABLES[n] = make_table(n)
    return _TABLES[n]


def make_task(table, m, hit, seed):
    """m handles in no particular order: about `hit` of them in the table, duplicates, the extremes"""
    rng = np.random.default_rng(seed)
    if m == 0:
        return np.zeros(0, np.int64)
    hits = table[rng.integers(0, table.size, m)] if table.size else np.zeros(m, np.int64)
    # misses: neighbours of table handles that are not in the table, and far values
    miss = rng.integers(-(1 << 62), 1 << 62, m).astype(np.int64)
    if table.size:
        near = table[rng.integers(0, table.size, m)]
        near = np.where(near < I64_MAX, near + 1, near - 1)
        miss = np.where(rng.random(m) < 0.5, near, miss)
        miss = miss[~np.isin(miss, table)]
        if miss.size == 0:
            miss = np.array([12345], np.int64)[~np.isin([12345], table)]
        miss = miss[rng.integers(0, miss.size, m)] if miss.size else hits
    take_hit = rng.random(m) < hit if table.size else np.zeros(m, bool)
    task = np.where(take_hit, hits, miss).astype(np.int64)
    if m >= 8:
        task[m // 2] = task[0]  # a duplicate whatever the draw
        task[1], task[m - 1] = I64_MAX, I64_MIN
    return task


class DevArr:
    """an int64 device array between two guard zones"""

    def __init__(self, ctx, n, init=None):
        self.ctx, self.n = ctx, n
        self.base = ctx.alloc((n + 2 * GUARD) * 8)
        host = np.full(n + 2 * GUARD, PATTERN, dtype=np.int64)
        if init is not None:
            host[GUARD:GUARD + n] = init
        ctx.h2d(self.base, host)
        self.ptr = self.base + GUARD * 8

    def read(self):
        host = np.zeros(self.n + 2 * GUARD, np.int64)
        self.ctx.d2h(host, self.base)
        return host

    def free(self):
        self.ctx.free(self.base)


class Lookup:
    def __init__(self, ctx, table):
        self.ctx, self.lib, self.table = ctx, ctx.lib, table
        self.dev = ctx.alloc(max(table.size, 1) * 8)
        if table.size:
            ctx.h2d(self.dev, table)
        h = C.c_void_p()
        st = self.lib.tsq_lookup_create(ctx.h, C.c_void_p(self.dev), table.size, abi.COL_DEVICE, C.byref(h))
        if st != abi.OK:
            ctx.free(self.dev)
            self.dev = None
            assert not h.value, "a failed create must not hand out a handle"
            raise _lib.TsqError(st, _lib.last_error(ctx.h))
        self.h = h

    def task_host(self, task, keep_order):
        n = task.size
        rows = np.full(n + 2 * GUARD, PATTERN, np.int64)
        hs = np.full(n + 2 * GUARD, PATTERN, np.int64)
        nf = C.c_int64(-1)
        inp = np.ascontiguousarray(task)
        _lib.check(self.lib.tsq_lookup_task(self.h, inp.ctypes.data_as(C.c_void_p), n, 0, int(keep_order), C.c_void_p(rows.ctypes.data + GUARD * 8),
                                            C.c_void_p(hs.ctypes.data + GUARD * 8), C.byref(nf)), self.h)
        assert (inp == task).all()
        return self._cut(rows, hs, nf.value, n)

    def task_dev(self, task, keep_order):
        n = task.size
        d_in, d_rows, d_hs = DevArr(self.ctx, n, task), DevArr(self.ctx, n), DevArr(self.ctx, n)
        try:
            nf = C.c_int64(-1)
            _lib.check(self.lib.tsq_lookup_task(self.h, C.c_void_p(d_in.ptr), n, abi.COL_DEVICE, int(keep_order), C.c_void_p(d_rows.ptr), C.c_void_p(d_hs.ptr),
                                                C.byref(nf)), self.h)
            assert (d_in.read()[GUARD:GUARD + n] == task).all(), "the task's handles were changed"
            return self._cut(d_rows.read(), d_hs.read(), nf.value, n)
        finally:
            for d in (d_in, d_rows, d_hs):
                d.free()

    @staticmethod
    def _cut(rows, hs, nf, n):
        assert 0 <= nf <= n
        for a in (rows, hs):  # the guards and everything beyond n_found stay untouched
            assert (a[:GUARD] == PATTERN).all() and (a[GUARD + nf:] == PATTERN).all()
        return rows[GUARD:GUARD + nf].copy(), hs[GUARD:GUARD + nf].copy()

    def stats(self):
        a, b, c, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_lookup_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(ms)), self.h)
        return a.value, b.value, c.value, ms.value

    def close(self):
        if self.h:
            self.lib.tsq_lookup_destroy(self.h)
            self.h = None
        if self.dev:
            self.ctx.free(self.dev)
            self.dev = None


def check_task(lk, task, keep_order, dev):
    got_rows, got_hs = (lk.task_dev if dev else lk.task_host)(task, keep_order)
    want_rows, want_hs = LR.lookup_task(lk.table, task, keep_order)
    assert got_rows.tolist() == want_rows.tolist() and got_hs.tolist() == want_hs.tolist(), (lk.table.size, task.size, keep_order, dev)
    if got_rows.size:
        assert (lk.table[got_rows] == got_hs).all()
    return got_rows.size


@pytest.mark.parametrize("stride", STRIDES)
@pytest.mark.parametrize("n_table", TABLE_SIZES)
def test_task_equals_the_restatement(ctx, stride, n_table):
    if stride is not None:
        ctx.set_knob(abi.KNOB_LOOKUP_STRIDE, stride)
    table = table_of(n_table)
    lk = Lookup(ctx, table)
    try:
        tasks = handles = found = 0
        for i, m in enumerate(TASK_SIZES):
            big = m >= 2049
            for hit in ((0.5,) if big and n_table not in (4097, 70001) else (0.0, 0.5, 1.0)):
                task = make_task(table, m, hit, 7 * i + int(hit * 10))
                for keep in (0, 1):
                    found += check_task(lk, task, keep, dev=(i + keep) % 2 == 0)
                    tasks += 1
                    handles += m
        st = lk.stats()
        assert st[:3] == (tasks, handles, found) and st[3] >= 0
    finally:
        lk.close()


def test_host_and_device_placement_both_orders(ctx):
    table = table_of(4097)
    lk = Lookup(ctx, table)
    try:
        task = make_task(table, 2049, 0.5, 3)
        for keep in (0, 1):
            for dev in (False, True):
                assert check_task(lk, task, keep, dev) > 0
        # every handle of the table, reversed: all hits, keep_order returns the reversed ordinals
        rows, hs = lk.task_dev(table[::-1].copy(), 1)
        assert rows.tolist() == list(range(table.size - 1, -1, -1)) and (hs == table[::-1]).all()
        rows, hs = lk.task_host(table[::-1].copy(), 0)
        assert rows.tolist() == list(range(table.size)) and (hs == table).all()
    finally:
        lk.close()


def test_duplicates_and_extremes(ctx):
    ctx.set_knob(abi.KNOB_LOOKUP_STRIDE, 2)
    table = np.array([I64_MIN, I64_MIN + 1, -1, 0, 1, I64_MAX - 1, I64_MAX], dtype=np.int64)
    lk = Lookup(ctx, table)
    try:
        task = np.array([I64_MAX, 0, 5, I64_MIN, 0, I64_MAX, -2, I64_MIN, 0], dtype=np.int64)
        rows, hs = lk.task_host(task, 1)  # the pinned departure: every occurrence at its own position
        assert rows.tolist() == [6, 3, 0, 3, 6, 0, 3] and hs.tolist() == [I64_MAX, 0, I64_MIN, 0, I64_MAX, I64_MIN, 0]
        rows, hs = lk.task_dev(task, 0)  # ascending, one entry per occurrence
        assert rows.tolist() == [0, 0, 3, 3, 3, 6, 6]
        unsigned = LR.as_i64([(1 << 63) - 1, 1 << 63, (1 << 64) - 1])  # an unsigned PK: raw bytes, signed order
        rows, hs = lk.task_host(unsigned, 0)
        assert rows.tolist() == [0, 2, 6] and hs.tolist() == [I64_MIN, -1, I64_MAX]
    finally:
        lk.close()


@pytest.mark.parametrize("bad", ["equal", "descending", "last_pair", "wrapped_unsigned"])
def test_table_not_ascending_is_refused(ctx, bad):
    t = np.arange(5000, dtype=np.int64) * 3
    if bad == "equal":
        t[2500] = t[2499]
    elif bad == "descending":
        t = t[::-1].copy()
    elif bad == "last_pair":
        t[-1] = t[-2] - 1
    else:
        t = LR.as_i64([1, (1 << 63) - 1, 1 << 63])  # ascending as unsigned numbers only
    with pytest.raises(_lib.TsqError) as e:
        Lookup(ctx, t).close()
    assert e.value.status == abi.ERR_INVALID and "table handles not ascending" in str(e.value)


def test_cancel_and_the_argument_contract(ctx):
    lib = ctx.lib
    h = C.c_void_p()
    host = np.arange(4, dtype=np.int64)
    assert lib.tsq_lookup_create(ctx.h, host.ctypes.data_as(C.c_void_p), 4, 0, C.byref(h)) == abi.ERR_INVALID and not h.value  # host table
    assert "device resident" in _lib.last_error(ctx.h)
    assert lib.tsq_lookup_create(ctx.h, None, 4, abi.COL_DEVICE, C.byref(h)) == abi.ERR_INVALID
    assert lib.tsq_lookup_create(ctx.h, None, -1, abi.COL_DEVICE, C.byref(h)) == abi.ERR_INVALID
    assert lib.tsq_lookup_create(ctx.h, None, 0, abi.COL_DEVICE, None) == abi.ERR_INVALID
    lk = Lookup(ctx, table_of(257))
    try:
        nf = C.c_int64(7)
        out = np.zeros(4, np.int64)
        p = out.ctypes.data_as(C.c_void_p)
        assert lib.tsq_lookup_task(lk.h, None, 4, 0, 0, p, p, C.byref(nf)) == abi.ERR_INVALID and nf.value == 0
        assert lib.tsq_lookup_task(lk.h, p, 4, 0, 0, None, p, C.byref(nf)) == abi.ERR_INVALID
        assert lib.tsq_lookup_task(lk.h, p, 4, 0, 0, p, None, C.byref(nf)) == abi.ERR_INVALID
        assert lib.tsq_lookup_task(lk.h, p, 4, 0, 0, p, p, None) == abi.ERR_INVALID
        assert lib.tsq_lookup_task(lk.h, p, -1, 0, 0, p, p, C.byref(nf)) == abi.ERR_INVALID
        assert lib.tsq_lookup_task(lk.h, p, 1 << 31, 0, 0, p, p, C.byref(nf)) == abi.ERR_UNSUPPORTED
        assert lib.tsq_lookup_task(lk.h, None, 0, 0, 1, None, None, C.byref(nf)) == abi.OK and nf.value == 0  # n = 0 needs no buffers
        assert lib.tsq_lookup_task(None, p, 4, 0, 0, p, p, C.byref(nf)) == abi.ERR_INVALID
        assert lib.tsq_lookup_stats(None, None, None, None, None) == abi.ERR_INVALID and lib.tsq_lookup_cancel(None) == abi.ERR_INVALID
        assert check_task(lk, lk.table[:10].copy(), 1, False) == 10
        assert lib.tsq_lookup_cancel(lk.h) == abi.OK
        nf.value = 5
        assert lib.tsq_lookup_task(lk.h, p, 4, 0, 0, p, p, C.byref(nf)) == abi.ERR_CANCELLED and nf.value == 0
        assert "cancelled" in _lib.last_error(lk.h)
        assert lib.tsq_lookup_task(lk.h, None, 0, 0, 0, None, None, C.byref(nf)) == abi.ERR_CANCELLED
    finally:
        lk.close()
    lib.tsq_lookup_destroy(None)
