"""Shared by the GPU tests of the transaction buffer and by smoke(): lists of pushes (tests/membuf_cases.py) through
tinysql_amd.kv.MemBuffer, host or device arrays, and the finished buffer against the dict model (tests/membuf_ref.py) — every entry's
op, key and value bytes, the counts, the size, the primary; then the buffer's own request through the MVCC writes against the model
of their write side."""
import numpy as np

from tests import membuf_ref as MR
from tests import mvcc_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import mvcc_write_ref as W
from tinysql_amd import kv
from tinysql_amd import mvcc as M
from tinysql_amd.dupcheck import DevArray


def pack(cells):
    offs = np.zeros(len(cells) + 1, dtype=np.int64)
    if cells:
        offs[1:] = np.cumsum([len(c) for c in cells])
    return np.frombuffer(b"".join(cells), dtype=np.uint8).copy(), offs


def push(mb, kind, keys, values=None, device=False, fixed=False):
    """one push of packed arrays; device: uploaded first and pushed as TSQ_COL_DEVICE, then freed — a push copies.  fixed: keys of one
    length through the NULL-offsets form"""
    kb, ko = pack(list(keys))
    vb, vo = pack(list(values)) if kind == MR.SET else (np.zeros(0, np.uint8), None)
    n = len(keys)
    if fixed:
        assert len({len(k) for k in keys}) <= 1
    if not device:
        mb.push_packed(kind, kb, None if fixed else ko, kb.size, n, vb if kind == MR.SET else None, vo, vb.size)
        return
    tmp = [DevArray(mb.ctx, a) for a in (kb, ko, vb, vo if vo is not None else np.zeros(1, np.int64))]
    try:
        mb.push_packed(kind, tmp[0].p, None if fixed else tmp[1].p, kb.size, n, tmp[2].p if kind == MR.SET else None, tmp[3].p if kind == MR.SET else None,
                       vb.size, device=True)
    finally:
        for t in tmp:
            t.free()


def fill(mb, pushes, device=False, fixed=False):
    for kind, keys, values in pushes:
        if keys:
            push(mb, kind, keys, values, device, fixed)


def check_finished(mb, model):
    """finish() and the read-back entries against Model.finish() -> the result dict"""
    want = model.finish()
    got = mb.finish()
    assert mb.entries() == want["entries"]
    assert {k: got[k] for k in ("n_entries", "puts", "dels", "locks", "size", "primary_index")} == dict(
        n_entries=len(want["entries"]), puts=want["puts"], dels=want["dels"], locks=want["locks"], size=want["size"], primary_index=want["primary_index"])
    assert mb.Len() == len(want["entries"]) and mb.Size() == want["size"]
    return got


def run_case(ctx, pushes, device=False, fixed=False, **limits):
    """a fresh buffer over the pushes, checked -> (the open kv.MemBuffer, the model, the result)"""
    mb = kv.MemBuffer(ctx, **limits)
    try:
        fill(mb, pushes, device, fixed)
        model = MR.replay(pushes)
        return mb, model, check_finished(mb, model)
    except BaseException:
        mb.close()
        raise


def commit_and_compare(ctx, mb, model, store_model, start_ts, commit_ts, ttl=3):
    """the buffer through mvcc.write_membuffer on a writable store of store_model, and the same mutations through the model of the write
    side: the full export of the next store equals the model's.  store_model is updated in place."""
    ms = WG.open_rw(ctx, store_model)
    try:
        want = model.finish()
        nxt = M.write_membuffer(ms, mb, start_ts, commit_ts, ttl)
        try:
            if want["entries"]:
                muts = [(op, k, v) for op, k, v in want["entries"]]
                v1, ok1 = W.prewrite(store_model, muts, want["primary"], start_ts, ttl)
                v2, ok2 = W.commit(store_model, [k for _, k, _ in muts], start_ts, commit_ts)
                assert ok1 and ok2, (v1, v2)
            WG.compare_store(nxt, store_model)
        finally:
            if nxt is not ms:
                nxt.close()
    finally:
        ms.close()


def empty_store():
    return R.Store()
