"""GPU: the union scan inside a device-resident plan — the stored rows of a table (record keys + rowcodec values) through
coprocessor.tableScanExec, GpuUnionScanExec and GpuHashAggExec, no host copy between them.  2^16 committed rows, 1000 of them deleted
and 1000 rows added by the transaction; the groups are compared with the same plan through tests/unionscan_ref.py and with numpy."""
import numpy as np
import pytest

from tests.unionscan_ref import UnionScanRef
from tinysql_amd import _abi as abi
from tinysql_amd import coprocessor as cop
from tinysql_amd import executor as X
from tinysql_amd import gpu_pipeline as P
from tinysql_amd import rowcodec as RC
from tinysql_amd import tablecodec as TC
from tinysql_amd.chunk import Chunk, Column

pytestmark = pytest.mark.gpu

TABLE_ID = 77
# the scan's schema: (g, v, handle) — the handle comes out of the record key
COLUMNS = [RC.ColInfo(1, RC.TypeLonglong), RC.ColInfo(2, RC.TypeLonglong), RC.ColInfo(-1, RC.TypeLonglong, IsPKHandle=True)]
TYPES = [abi.I64, abi.I64, abi.I64]


def test_table_scan_union_scan_hash_agg(ctx):
    rng = np.random.default_rng(77)
    n = 1 << 16
    handles = np.sort(rng.choice(np.arange(-200_000, 200_000, 2), n, replace=False)).astype(np.int64)  # even handles, key order
    g = rng.integers(0, 300, n)
    v = rng.integers(-1000, 1000, n)
    nn = rng.random(n) > 0.05
    committed = Chunk([Column(abi.I64, g), Column(abi.I64, v, nn)])
    vals, offs = TC.EncodeRow(ctx, committed, [1, 2])
    keys = TC.EncodeRowKeysWithHandles(ctx, TABLE_ID, handles)
    deleted = rng.choice(handles, 1000, replace=False)
    added_h = np.sort(rng.choice(np.arange(-200_001, 200_001, 2), 1000, replace=False)).astype(np.int64)  # odd handles
    ag, av = rng.integers(290, 320, 1000), rng.integers(-1000, 1000, 1000)  # some groups exist only in the transaction
    dirty = X.DirtyTable()
    for h in added_h:
        dirty.AddRow(h)
    for h in deleted:
        dirty.DeleteRow(h)
    added = Chunk([Column(abi.I64, ag), Column(abi.I64, av), Column(abi.I64, added_h)])
    aggs = [X.AggFuncDesc(abi.AGG_FIRSTROW, 0), X.AggFuncDesc(abi.AGG_COUNT, -1), X.AggFuncDesc(abi.AGG_SUM, 1), X.AggFuncDesc(abi.AGG_COUNT, 1)]

    scan = cop.tableScanExec(ctx, COLUMNS, keys, vals, offs, batch_rows=1 << 14)
    us = P.GpuUnionScanExec(ctx, scan, dirty, added, [], 2, False, pull_rows=1 << 15)
    agg = P.GpuHashAggExec(ctx, us, [0], aggs)
    got = sorted(r for ch in P.drain_device(agg) for r in ch.rows())

    # the same plan through the Python restatement: the scan's rows, the union scan row by row, the groups in a dict
    snap = list(zip(g.tolist(), [x if ok else None for x, ok in zip(v.tolist(), nn.tolist())], handles.tolist()))
    rows = UnionScanRef(TYPES, dirty.addedRows, dirty.deletedRows, added.rows(), [], 2, False).run([snap])
    assert len(rows) == n - 1000 + 1000 and [r[2] for r in rows] == sorted(r[2] for r in rows)
    groups = {}
    for gg, vv, _ in rows:
        c = groups.setdefault(gg, [0, 0, 0])
        c[0] += 1
        if vv is not None:
            c[1] += vv
            c[2] += 1
    want = sorted((k, c[0], c[1] if c[2] else None, c[2]) for k, c in groups.items())
    assert got == want

    # ... and with numpy on the columns
    keep = ~np.isin(handles, deleted)
    all_g = np.concatenate([g[keep], ag])
    all_v = np.concatenate([np.where(nn, v, 0)[keep], av])
    all_nn = np.concatenate([nn[keep], np.ones(1000, bool)])
    ks = np.unique(all_g)
    assert [r[0] for r in got] == ks.tolist()
    assert [r[1] for r in got] == [int((all_g == k).sum()) for k in ks]
    assert [r[2] or 0 for r in got] == [int(all_v[(all_g == k) & all_nn].sum()) for k in ks]
