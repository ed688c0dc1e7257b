"""GPU parity of the mem readers' view of the transaction buffer — tsq_membuf_scan / scan_points / fetch / dirty / dirty_fetch and
tsq_unionscan_create_dev — with tests/memread_ref.py through the C-ABI: every pair's key and value bytes in order, the counts per range,
positions and skipped deletes, host and device ranges, ascending and descending; the refusals; the dirty handles of a table; and the
device-built handle set against the host-built one on the union scan's own cases.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from tests import membuf_cases as MC
from tests import membuf_gpu_helpers as BG
from tests import membuf_ref as MR
from tests import memread_cases as K
from tests import memread_ref as R
from tests import test_unionscan_gpu as UG
from tests import unionscan_cases as UC
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import executor as X
from tinysql_amd import kv
from tinysql_amd.dupcheck import DevArray

pytestmark = pytest.mark.gpu

TID = 41
flip = R.flip


def mixed_pushes():
    """19-byte record keys of three tables and variable-length index keys in one buffer; values of 1, 63, 64, 65 and 300 bytes (both sides
    of the wave-copy threshold); deletes, lock-only keys, a key written twice"""
    rng = np.random.default_rng(61)
    hs = np.unique(np.concatenate([np.array([-(1 << 63), -1, 0, 1, (1 << 63) - 1], dtype=np.int64), rng.integers(-(1 << 40), 1 << 40, 300)]))
    rec = MC.record_keys(TID, hs)
    rec = [rec[i] for i in rng.permutation(len(rec))]
    ix1 = [R.index_prefix(TID, 1) + b"\x03" + flip(int(h) % 97) + flip(h) for h in hs[:120]]
    ix2 = [R.index_prefix(TID, 2) + b"\x01" + (b"s%d" % (int(h) % 1009)) * (1 + int(h) % 3) + b"\xf9" for h in hs[:120]]
    return [MC.sets(rec, 0), MC.sets(ix1, 400, 1), MC.sets(ix2, 600), MC.deletes(rec[10:40] + ix1[5:9]), MC.locks(MC.record_keys(TID, [5000, 5001, 5002]) + rec[:3]),
            MC.deletes(MC.record_keys(TID, [7000, 7001, 7002])),
            MC.sets(MC.record_keys(TID - 1, [1, 2, 3]) + MC.record_keys(TID + 1, [4, 5]), 900, 64), MC.sets(rec[50:60], 1000, 65)]


@pytest.fixture(scope="module")
def mixed(ctx):
    pushes = mixed_pushes()
    mb, model, _ = BG.run_case(ctx, pushes, device=True)
    yield mb, model
    mb.close()


def scan_gpu(ctx, mb, ranges, desc, device):
    """-> (pairs, counts dict) of one scan + fetch; device: the ranges uploaded and passed as TSQ_COL_DEVICE"""
    if device:
        rb, ro = BG.pack([bytes(b) for r in ranges for b in r])
        tmp = [DevArray(ctx, rb), DevArray(ctx, ro)]
        try:
            p = mb.scan_packed(tmp[0].p, tmp[1].p, len(ranges), desc, device=True, want_counts=True)
        finally:
            for t in tmp:
                t.free()
    else:
        p = mb.scan(ranges, desc, want_counts=True)
    try:
        return p.to_host(), dict(p.scan, range_counts=list(p.counts))
    finally:
        p.free()


def same_as_model(want, got):
    pairs, counts = got
    assert pairs == want["pairs"]
    assert counts == dict(n_pairs=len(want["pairs"]), key_bytes=sum(len(k) for k, _ in want["pairs"]), value_bytes=sum(len(v) for _, v in want["pairs"]),
                          positions=want["positions"], skipped_dels=want["skipped_dels"], range_counts=want["range_counts"])


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_scan_edge_ranges_equal_the_model(ctx, mixed, device, desc):
    """a start and an end equal to a stored key, proper prefixes, extensions by 0x00, empty start, empty end, start >= end, overlapping and
    identical ranges — over record keys mixed with variable-length index keys, all five value lengths"""
    mb, model = mixed
    keys = [e[1] for e in R.entries(model)]
    assert {len(v) for _, _, v in R.entries(model)} >= {1, 63, 64, 65, 300} and len({len(k) for k in keys}) > 3
    rs = K.edge_ranges(keys)
    same_as_model(R.scan(model, rs, desc), scan_gpu(ctx, mb, rs, desc, device))
    one = [(R.record_prefix(TID), R.record_prefix(TID)[:-1] + b"s")]
    same_as_model(R.scan(model, one, desc), scan_gpu(ctx, mb, one, desc, device))


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_scan_zero_one_and_1025_ranges(ctx, mixed, device):
    mb, model = mixed
    keys = [e[1] for e in R.entries(model)]
    rng = np.random.default_rng(67)
    many = []
    for _ in range(1025):
        i = int(rng.integers(0, len(keys)))
        many.append((keys[i], keys[min(len(keys) - 1, max(0, i + int(rng.integers(-3, 12))))]))
    for ranges in ([], [(b"", b"")], many):
        for desc in (False, True):
            same_as_model(R.scan(model, ranges, desc), scan_gpu(ctx, mb, ranges, desc, device))


def test_scan_ranges_of_deletes_only_and_of_lock_only_keys(ctx, mixed):
    mb, model = mixed
    ents = R.entries(model)
    run = lambda op: next((ents[i][1], ents[j][1]) for i in range(len(ents)) for j in range(i + 2, len(ents)) if all(e[0] == op for e in ents[i:j])
                          and ents[j][0] != op)
    for op, dels in ((MR.OP_DEL, True), (MR.OP_LOCK, False)):
        a, b = run(op)
        want = R.scan(model, [(a, b)])
        assert want["pairs"] == [] and want["positions"] >= 2 and (want["skipped_dels"] == want["positions"]) == dels
        same_as_model(want, scan_gpu(ctx, mb, [(a, b)], False, False))
        same_as_model(R.scan(model, [(a, b)], True), scan_gpu(ctx, mb, [(a, b)], True, True))


def test_empty_buffer(ctx):
    mb = kv.MemBuffer(ctx)
    try:
        mb.finish()
        for ranges in ([], [(b"", b"")], [(b"a", b"b"), (b"", b"z")]):
            same_as_model(R.scan(MR.Model(), ranges), scan_gpu(ctx, mb, ranges, False, False))
            same_as_model(R.scan(MR.Model(), ranges, True), scan_gpu(ctx, mb, ranges, True, True))
        p = mb.scan_points([b"a", b"b"])
        assert p.to_host() == [] and p.scan["positions"] == 0
        p.free()
        assert mb.Iter() == []
        a, na, d, nd = mb.dirty_handles(TID)
        assert (na, nd) == (0, 0)
        ctx.free(a)
        ctx.free(d)
    finally:
        mb.close()


@pytest.mark.parametrize("desc", [False, True], ids=["asc", "desc"])
def test_3000_entries_in_one_range_cross_the_scan_tiles(ctx, desc):
    """3000 positions in one range and 6000 over two overlapping ones — more than one tile of the position scans, so tile carries are
    exercised; every third entry a delete, value lengths on both sides of the wave-copy threshold"""
    hs = list(range(-1500, 1500))
    keys = MC.record_keys(TID, hs)
    pushes = [MC.sets(keys, 0), MC.deletes(keys[::3])]
    mb, model, _ = BG.run_case(ctx, pushes, device=True, fixed=False)
    try:
        full = (R.record_prefix(TID), R.prefix_next(R.record_prefix(TID)))
        for ranges in ([full], [full, (keys[7], keys[2990]), full]):
            want = R.scan(model, ranges, desc)
            assert want["positions"] == sum((3000, 2983, 3000)[:len(ranges)]) and want["skipped_dels"] >= 1000
            same_as_model(want, scan_gpu(ctx, mb, ranges, desc, True))
        assert mb.Iter(keys[10], keys[14]) == [(k, v) for k, v in R.scan(model, [(keys[10], keys[14])])["pairs"]]
    finally:
        mb.close()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
def test_points_keep_the_input_order(ctx, mixed, device):
    """hits, misses, deleted keys, lock-only keys, a repeated key, keys beyond both ends; variable-length keys and, for record keys, the
    fixed-length (NULL offsets) form"""
    mb, model = mixed
    ents = R.entries(model)
    by_op = {op: [k for o, k, _ in ents if o == op] for op in (MR.OP_PUT, MR.OP_DEL, MR.OP_LOCK)}
    keys = by_op[MR.OP_PUT][::7] + by_op[MR.OP_DEL][:5] + by_op[MR.OP_LOCK][:3] + [b"\x00", b"\xff" * 30, ents[0][1][:-1], ents[-1][1] + b"\x00"]
    keys += [by_op[MR.OP_PUT][3]] * 3 + by_op[MR.OP_PUT][::-11]
    rec = [k for k in keys if len(k) == 19] + MC.record_keys(TID, [123456789, -(1 << 63) + 1])
    for ks, fixed in ((keys, False), (rec, True), ([], False)):
        kb, ko = BG.pack(ks)
        if device:
            tmp = [DevArray(ctx, kb), DevArray(ctx, ko)]
            p = mb.scan_points_packed(tmp[0].p, None if fixed else tmp[1].p, kb.size, len(ks), device=True)
            for t in tmp:
                t.free()
        else:
            p = mb.scan_points_packed(kb, None if fixed else ko, kb.size, len(ks))
        try:
            want = R.scan_points(model, ks)
            assert p.to_host() == want["pairs"] and p.scan["positions"] == want["positions"] and p.scan["skipped_dels"] == want["skipped_dels"]
        finally:
            p.free()


def raw_scan(mb, rb, ro, n, flags=0, desc=0, result=True):
    res = abi.MembufScanResult()
    st = mb.lib.tsq_membuf_scan(mb.h, C.c_void_p(kv.MemBuffer._ptr(rb)), C.c_void_p(kv.MemBuffer._ptr(ro)), n, flags, desc, C.byref(res) if result else None, None)
    return st, res


def test_refusals(ctx):
    mb = kv.MemBuffer(ctx)
    lib = ctx.lib
    try:
        rb, ro = BG.pack([b"a", b"z"])
        BG.push(mb, MR.SET, [b"k1", b"k2", b"k3"], [b"v" * 70, b"w", b"x" * 5])
        st, _ = raw_scan(mb, rb, ro, 1)
        assert st == abi.ERR_INVALID and "membuf: not finished" in _lib.last_error(mb.h)  # before a finish
        na, nd = C.c_int64(0), C.c_int64(0)
        assert lib.tsq_membuf_dirty(mb.h, TID, C.byref(na), C.byref(nd)) == abi.ERR_INVALID and "not finished" in _lib.last_error(mb.h)
        mb.finish()
        bufs = [DevArray(ctx, nbytes=256) for _ in range(4)]
        try:
            fetch = lambda kc, vc: lib.tsq_membuf_fetch(mb.h, C.c_void_p(bufs[0].p), kc, C.c_void_p(bufs[1].p), C.c_void_p(bufs[2].p), vc, C.c_void_p(bufs[3].p))
            assert fetch(256, 256) == abi.ERR_INVALID  # a fetch without a scan
            st, res = raw_scan(mb, rb, ro, 1)
            assert st == abi.OK and (res.n_pairs, res.key_bytes, res.value_bytes) == (3, 6, 76)
            for b in bufs:
                ctx.memset(b.p, 0xAB, 256)
            for kc, vc in ((res.key_bytes - 1, res.value_bytes), (res.key_bytes, res.value_bytes - 1)):  # a cap one byte short: nothing is written
                assert fetch(kc, vc) == abi.ERR_INVALID
                assert all((b.read(np.uint8, 256) == 0xAB).all() for b in bufs)
            assert fetch(res.key_bytes, res.value_bytes) == abi.OK
            assert bufs[0].read(np.uint8, 6).tobytes() == b"k1k2k3" and bufs[1].read(np.int64, 4).tolist() == [0, 2, 4, 6] and bufs[3].read(np.int64, 4).tolist() == [0, 70, 71, 76]
            assert (bufs[0].read(np.uint8, 256)[6:] == 0xAB).all() and (bufs[2].read(np.uint8, 256)[76:] == 0xAB).all()  # and nothing behind the pairs
            # a NULL result; bad offsets, host and device, ranges and points
            assert raw_scan(mb, rb, ro, 1, result=False)[0] == abi.ERR_INVALID
            for bad in (np.array([0, 2, 1], np.int64), np.array([-1, 0, 1], np.int64), np.array([1, 0, 2], np.int64)):
                assert raw_scan(mb, rb, bad, 1)[0] == abi.ERR_INVALID and "offsets" in _lib.last_error(mb.h)
                d = [DevArray(ctx, rb), DevArray(ctx, bad)]
                assert raw_scan(mb, d[0].p, d[1].p, 1, abi.COL_DEVICE)[0] == abi.ERR_INVALID and "offsets" in _lib.last_error(mb.h)
                pres = abi.MembufScanResult()
                assert lib.tsq_membuf_scan_points(mb.h, C.c_void_p(d[0].p), C.c_void_p(d[1].p), 2, 2, abi.COL_DEVICE, C.byref(pres)) == abi.ERR_INVALID
                for x in d:
                    x.free()
                assert fetch(256, 256) == abi.ERR_INVALID  # a failed scan leaves nothing to fetch
            assert raw_scan(mb, rb, ro, -1)[0] == abi.ERR_INVALID
            # after a later push: not finished again, for the scan, the fetch and the dirty handles
            assert raw_scan(mb, rb, ro, 1)[0] == abi.OK
            BG.push(mb, MR.DELETE, [b"k2"])
            assert raw_scan(mb, rb, ro, 1)[0] == abi.ERR_INVALID and "membuf: not finished" in _lib.last_error(mb.h)
            assert fetch(256, 256) == abi.ERR_INVALID
            assert lib.tsq_membuf_dirty_fetch(mb.h, None, None) == abi.ERR_INVALID
        finally:
            for b in bufs:
                b.free()
    finally:
        mb.close()


def test_second_finish_sees_both_pushes(ctx):
    mb = kv.MemBuffer(ctx)
    try:
        first = [MC.sets([b"b", b"d", b"f"], 0, 64), MC.deletes([b"c"])]
        BG.fill(mb, first)
        mb.finish()
        model = MR.replay(first)
        same_as_model(R.scan(model, [(b"", b"")]), scan_gpu(ctx, mb, [(b"", b"")], False, False))
        second = [MC.sets([b"a", b"c", b"e"], 10, 65), MC.deletes([b"d"]), MC.locks([b"g"])]
        BG.fill(mb, second)
        mb.finish()
        model = MR.replay(first + second)
        for desc in (False, True):
            want = R.scan(model, [(b"", b""), (b"c", b"f")], desc)
            same_as_model(want, scan_gpu(ctx, mb, [(b"", b""), (b"c", b"f")], desc, True))
        assert [k for k, _ in mb.Iter()] == [b"a", b"b", b"c", b"e", b"f"]
    finally:
        mb.close()


def dirty_gpu(ctx, mb, table_id):
    a, na, d, nd = mb.dirty_handles(table_id)
    try:
        out = (np.zeros(max(na, 1), np.int64), np.zeros(max(nd, 1), np.int64))
        if na:
            ctx.d2h(out[0][:na], a)
        if nd:
            ctx.d2h(out[1][:nd], d)
        return out[0][:na].tolist(), out[1][:nd].tolist()
    finally:
        ctx.free(a)
        ctx.free(d)


def test_dirty_handles_of_a_table(ctx):
    """record keys of table_id - 1 and table_id + 1 and index keys of table_id itself are present and not reported; INT64_MIN, -1, 0, 1 and
    INT64_MAX among the handles; PUT, DEL and lock-only entries each in the right list; a table with no entries; 700 handles cross a scan tile"""
    edge = [-(1 << 63), -1, 0, 1, (1 << 63) - 1]
    many = list(range(1000, 1700))
    pushes = [MC.sets(MC.record_keys(TID, edge + [7, 8, 9] + many), 0, 38), MC.deletes(MC.record_keys(TID, [8, 100, -5] + many[::2])), MC.locks(MC.record_keys(TID, [9, 200])),
              MC.sets(MC.record_keys(TID - 1, [1, 2]) + MC.record_keys(TID + 1, [3]), 50, 38), MC.deletes(MC.record_keys(TID + 1, [4])),
              MC.sets([R.index_prefix(TID, 1) + b"\x03abc", R.index_prefix(TID, 2) + flip(5)], 60, 8), MC.sets(MC.record_keys(TID, [100]), 70, 5),
              MC.deletes(MC.record_keys(TID, [7]))]
    mb, model, _ = BG.run_case(ctx, pushes, device=True)
    try:
        want = R.dirty_sets(model, TID)
        assert 100 in want[0] and 7 in want[1] and 200 not in want[0] + want[1] and len(want[1]) > 350
        assert dirty_gpu(ctx, mb, TID) == (want[0], want[1])
        assert dirty_gpu(ctx, mb, TID + 1) == ([3], [4]) and dirty_gpu(ctx, mb, TID - 1) == ([1, 2], [])
        assert dirty_gpu(ctx, mb, TID + 7) == ([], []) and dirty_gpu(ctx, mb, -(1 << 63)) == ([], []) and dirty_gpu(ctx, mb, (1 << 63) - 1) == ([], [])
        BG.push(mb, MR.SET, [R.record_key(TID, 5) + b"\x00"], [b"v"])  # a 20-byte key inside the record range
        mb.finish()
        na, nd = C.c_int64(0), C.c_int64(0)
        assert ctx.lib.tsq_membuf_dirty(mb.h, TID, C.byref(na), C.byref(nd)) == abi.ERR_INVALID and "invalid key" in _lib.last_error(mb.h)
        assert dirty_gpu(ctx, mb, TID + 1) == ([3], [4])  # another table of the same buffer is still answered
    finally:
        mb.close()


# ------------------------------------------------------------------------------------------------ tsq_unionscan_create_dev
class DevHandle(UG.Handle):
    """tests/test_unionscan_gpu.Handle with the set built on the device from uploaded handle arrays"""

    def __init__(self, ctx, cs, cap=1024):
        self.ctx, self.lib, self.cs, self.cap = ctx, ctx.lib, cs, cap
        cfg = X.unionscan_cfg(cs.types, cs.used_index, cs.handle_idx, cs.desc, cap)
        arrs = [DevArray(ctx, np.array(hs, dtype=np.int64)) for hs in (cs.added_handles, cs.deleted_handles)]
        try:
            h = C.c_void_p()
            _lib.check(ctx.lib.tsq_unionscan_create_dev(ctx.h, C.byref(cfg), C.c_void_p(arrs[0].p), len(cs.added_handles), C.c_void_p(arrs[1].p),
                                                        len(cs.deleted_handles), C.byref(h)), ctx.h)
            self.h = h
        finally:
            for a in arrs:
                a.free()


def both_creates(ctx, monkeypatch, cs, **kw):
    host = UG.run_abi(ctx, cs, **kw)
    with monkeypatch.context() as m:
        m.setattr(UG, "Handle", DevHandle)
        dev = UG.run_abi(ctx, cs, **kw)
    assert UC.canon(cs.types, dev) == UC.canon(cs.types, host) == UC.canon(cs.types, cs.want()), cs.name
    return dev


def dup_case():
    """duplicate handles inside and across the two lists (the host build stores a handle once, the device build once per occurrence)"""
    cs = UC.table_case("alternate", 513)
    cs.added_handles = cs.added_handles * 3 + cs.added_handles[:7]
    cs.deleted_handles = [r[0] for r in cs.snapshot[::5]] * 2 + cs.added_handles[:20]
    return UC.Case(cs.types, cs.handle_idx, cs.used_index, cs.desc, cs.snapshot, cs.added_rows, cs.added_handles, cs.deleted_handles, "duplicates")


CREATE_CASES = [UC.colliding_case(), dup_case(), UC.table_case("m0", 257), UC.table_case("all_deleted", 1025), UC.table_case("runs_1000", 4097),
                UC.edge_handle_case(abi.I64, False, 0), UC.edge_handle_case(abi.I64, True, 1), UC.edge_handle_case(abi.U64, False, 1),
                UC.one_key_case(abi.BYTES, True), UC.multi_key_case(4, False)] + [UC.txn_case(UC.SNAP, g[0], g[1], g[2]) for g in UC.GOLDEN[::3]]


@pytest.mark.parametrize("cs", CREATE_CASES, ids=[c.name + str(i) for i, c in enumerate(CREATE_CASES)])
def test_create_dev_answers_as_create(ctx, monkeypatch, cs):
    both_creates(ctx, monkeypatch, cs)
    both_creates(ctx, monkeypatch, cs, cuts=[3, 60, 64], check_prefix=True)


def test_create_dev_with_empty_lists_and_bad_arguments(ctx, monkeypatch):
    cs = UC.Case(UC.T3, 0, [], False, [UC.row3(h) for h in range(10)], [], [], [], "no-handles")  # no handles at all: nothing is probed
    assert both_creates(ctx, monkeypatch, cs) == cs.snapshot
    cs = UC.Case(UC.T3, 0, [], False, [UC.row3(h) for h in range(10)], [], [], [3], "one-deleted")
    assert len(both_creates(ctx, monkeypatch, cs)) == 9
    cfg = X.unionscan_cfg(UC.T3, [], 0, False, 1024)
    h = C.c_void_p()
    assert ctx.lib.tsq_unionscan_create_dev(ctx.h, C.byref(cfg), None, 3, None, 0, C.byref(h)) == abi.ERR_INVALID and not h.value
    assert ctx.lib.tsq_unionscan_create_dev(ctx.h, C.byref(cfg), None, -1, None, 0, C.byref(h)) == abi.ERR_INVALID
