"""Shared by the GPU tests of the union store and by smoke(): a model store (tests/mvcc_ref.py) and a model buffer (tests/membuf_ref.py)
uploaded, one read answered by the device and by tests/unionstore_ref.py — pairs, curIsDirty flags, per-range counts, the result's
counts, or the lock's key and the pairs before it — compared exactly."""
import numpy as np

from tests import membuf_gpu_helpers as BG
from tests import mvcc_gpu_helpers as MG
from tests import unionstore_cases as K
from tests import unionstore_ref as U
from tinysql_amd import _abi as abi
from tinysql_amd import kv
from tinysql_amd import mvcc as M


class Opened:
    """store + buffer (pushes None: no buffer at all) on the device with the union store over them, and the model's view"""

    def __init__(self, ctx, store, pushes, ts=K.READ_TS, device_pushes=False):
        self.ctx, self.store, self.ts = ctx, store, ts
        self.dirty = U.Dirty(K.model_of(pushes))
        self.ms = MG.open_store(ctx, store)
        self.mb = None
        try:
            if pushes is not None:
                self.mb = kv.MemBuffer(ctx)
                BG.fill(self.mb, pushes, device_pushes)
                self.mb.finish()
            self.us = kv.UnionStore(ctx, self.ms, self.mb, ts)
        except BaseException:
            self.close(False)
            raise

    def close(self, with_us=True):
        if with_us:
            self.us.close()
        if self.mb is not None:
            self.mb.close()
        self.ms.close()

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


def gpu_answer(o, ranges, desc=False, limit=-1):
    try:
        p = o.us.scan(ranges, desc, limit, want_counts=True)
    except M.ErrLocked as e:
        return ("locked", e.RawKey, e.n_pairs), None
    try:
        fb = p.from_buffer.read(np.uint8, p.n).tolist()
        assert p.scan["from_buffer"] == sum(fb)
        return ("ok", p.to_host(), fb, p.counts), p.scan
    finally:
        p.free()


def check(o, ranges, desc=False, limit=-1):
    """one scan against the model -> (the model's answer, the route that ran)"""
    want = K.answer(o.store, o.dirty, ranges, o.ts, desc, limit)
    got, res = gpu_answer(o, ranges, desc, limit)
    assert got == want, (ranges[:3], desc, limit, got[0], want[0], got[2] if got[0] == "locked" else len(got[1]), want[2] if want[0] == "locked" else len(want[1]))
    route = o.us.stats()["last_route"]
    if want[0] == "ok":
        assert (res["n_pairs"], res["key_bytes"], res["value_bytes"]) == (len(want[1]), sum(len(k) for k, _ in want[1]), sum(len(v) for _, v in want[1]))
        if limit != 0:
            st = U.scan_stats(o.store, o.dirty, ranges, o.ts)
            assert {k: res[k] for k in st} == st, (ranges[:3], desc, limit, route)
    return want, route


def gpu_points(o, keys, fixed=False):
    kb, ko = BG.pack([bytes(k) for k in keys])
    try:
        found, p = o.us.get_packed(kb, None if fixed else ko, kb.size, len(keys))
    except M.ErrLocked as e:
        return ("locked", e.RawKey, e.n_pairs)
    try:
        pairs = iter(p.to_host())
        out = []
        for k, f in zip(keys, found):
            if f:
                pk, pv = next(pairs)
                assert pk == k
                out.append(pv)
            else:
                out.append(None)
        assert next(pairs, None) is None and p.n == int(found.sum())
        fb = p.from_buffer.read(np.uint8, p.n).tolist()
        held = dict(o.dirty.pairs)
        assert fb == [1 if k in held else 0 for k, f in zip(keys, found) if f]
        return ("ok", out)
    finally:
        p.free()


def check_points(o, keys, fixed=False):
    want = K.point_answer(o.store, o.dirty, keys, o.ts)
    got = gpu_points(o, keys, fixed)
    assert got == want, (keys[:4], got[0], want[0])
    assert o.us.stats()["last_route"] == abi.UNION_ROUTE_POINTS
    return want
