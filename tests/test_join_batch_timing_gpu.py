"""Which partitioned probe batches of a join handle record HIP events (TSQ_KNOB_JOIN_BATCH_TIMING, csrc/tsq_join.hip batch_begin):
batch b is timed iff b % N == N - 1 (default N = 4; 1: every batch; 0: none), an untimed batch records nothing, and tsq_join_stats
sums only the slots that timed batches among the 32 most recent wrote — never a slot an older batch left behind.  COUNT(*) on the
packed route, 2^16 unique build keys, device batches of 4096 probe rows; the count is what numpy counts whatever is timed.
"""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd.chunk import Chunk, Column

from . import gpu_helpers as G
from . import helpers as H

pytestmark = pytest.mark.gpu

N_BUILD = 1 << 16
BATCH = 4096


def _chunk(keys):
    return Chunk([Column(abi.I64, keys), Column(abi.I64, np.arange(len(keys)))])


def _run(ctx, batches, knob):
    """`batches` device batches through one handle; (count, expected count, statistics)"""
    rng = np.random.default_rng(13)
    bk = rng.permutation(N_BUILD).astype(np.int64) + 1000
    pk = rng.integers(1000 - N_BUILD // 4, 1000 + N_BUILD + N_BUILD // 4, (batches, BATCH)).astype(np.int64)
    want = int(np.count_nonzero((pk >= 1000) & (pk < 1000 + N_BUILD)))
    lib = ctx.lib
    knobs = {} if knob is None else {"JOIN_BATCH_TIMING": knob}
    bufs = []
    with ctx.knobs(**knobs):
        h = C.c_void_p()
        cfg = H.join_cfg([abi.I64, abi.I64], [abi.I64, abi.I64], [0], [0], abi.JOIN_INNER, 1)
        _lib.check(lib.tsq_join_create(ctx.h, C.byref(cfg), C.byref(h)), ctx.h)
        try:
            _lib.check(lib.tsq_join_set_radix(h, abi.RADIX_FORCE), h)
            _lib.check(lib.tsq_join_set_key_packing(h, abi.RADIX_FORCE), h)
            G.push_chunked(lib.tsq_join_build_push, h, _chunk(bk), 1 << 24)
            _lib.check(lib.tsq_join_build_finish(h), h)
            _lib.check(lib.tsq_join_set_count_only(h, 1), h)
            kd, vd = ctx.alloc(pk.nbytes + 64), ctx.alloc(BATCH * 8 + 64)
            bufs += [kd, vd]
            ctx.h2d(kd, np.ascontiguousarray(pk))
            ctx.h2d(vd, np.zeros(BATCH, np.int64))
            for b in range(batches):
                cols = (abi.Col * 2)()
                for i, p in enumerate((kd + b * BATCH * 8, vd)):
                    cols[i].data, cols[i].length, cols[i].elem_size, cols[i].type, cols[i].flags = p, BATCH, 8, abi.I64, abi.COL_DEVICE
                _lib.check(lib.tsq_join_probe_push(h, cols, 2, BATCH, None), h)
            c = C.c_int64(0)
            _lib.check(lib.tsq_join_count(h, C.byref(c)), h)
            st = abi.Stats()
            _lib.check(lib.tsq_join_stats(h, C.byref(st)), h)
        finally:
            lib.tsq_join_destroy(h)
            for p in bufs:
                ctx.free(p)
    assert st.probe_route == abi.ROUTE_PACKED and st.radix_batches == batches
    return c.value, want, st


@pytest.mark.parametrize("batches,knob,timed", [(9, None, 2), (9, 1, 9), (9, 0, 0), (40, None, 8), (40, 1, 32)])
def test_timed_batches(ctx, batches, knob, timed):
    got, want, st = _run(ctx, batches, knob)
    assert got == want
    assert st.radix_timed_batches == timed
    if timed == 0:
        assert st.partition_kernel_ms_sum == 0 and st.radix_probe_kernel_ms_sum == 0
    else:
        assert st.partition_kernel_ms_sum > 0 and st.radix_probe_kernel_ms_sum > 0
        assert st.partition_kernel_ms > 0 and st.probe_kernel_ms >= st.partition_kernel_ms


def test_count_is_the_same_whatever_is_timed(ctx):
    runs = [_run(ctx, 9, knob) for knob in (None, 1, 0)]
    assert len({got for got, _, _ in runs}) == 1
    assert all(got == want for got, want, _ in runs)
