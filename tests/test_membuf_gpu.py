"""GPU parity of the transaction buffer (tsq_membuf_create / push / finish / request / get / destroy) with the dict model of
tests/membuf_ref.py, through the C-ABI: every entry's op, key and value bytes, the counts, size and primary — over the grid of counts,
key lengths, value lengths, key sets and write orders of tests/membuf_cases.py, host and device inputs — then the buffer's own request
through tsq_mvcc_prewrite / commit against the model of the write side.  Every comparison is exact."""
import ctypes as C

import numpy as np
import pytest

from tests import membuf_cases as MC
from tests import membuf_gpu_helpers as BG
from tests import membuf_ref as MR
from tests import mvcc_ref as R
from tests import mvcc_write_gpu_helpers as WG
from tests import mvcc_write_ref as W
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import kv
from tinysql_amd import mvcc as M

pytestmark = pytest.mark.gpu

SMALL = MC.key_set_cases() + MC.order_cases()


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("name,pushes", SMALL, ids=[c[0] for c in SMALL])
def test_key_sets_and_orders_equal_the_model(ctx, name, pushes, device):
    mb, model, res = BG.run_case(ctx, pushes, device)
    try:
        keys = [k for _, ks, _ in pushes for k in ks]
        if len(set(keys)) > 1 and not all(a < b for a, b in zip(keys, keys[1:])):
            assert res["sort_passes"] > 0
        BG.commit_and_compare(ctx, mb, model, R.Store(), 10, 20)  # no "not strictly ascending": the request is what the prewrite asks for
    finally:
        mb.close()


@pytest.mark.parametrize("name,pushes", MC.count_cases(), ids=[c[0] for c in MC.count_cases()])
def test_counts_record_keys_fixed_length_form(ctx, name, pushes):
    """n = 0, 1, 2, 63..65, 255..257 and one key more than two tiles of the radix pass: record keys of shuffled handles through the
    NULL-offsets form, a tenth of them written twice (the second value stays)"""
    mb, model, res = BG.run_case(ctx, pushes, device=True, fixed=True)
    try:
        n = len(pushes[0][1])
        assert res["n_entries"] == n and res["puts"] == n
        BG.commit_and_compare(ctx, mb, model, R.Store(), 5, 6)
    finally:
        mb.close()


def edge_handles(rng, n):
    hs = np.concatenate([np.array([-(1 << 63), (1 << 63) - 1, -1, 0, 1], dtype=np.int64), rng.integers(-(1 << 62), 1 << 62, n - 5)])
    return np.unique(hs)


def test_record_streams(ctx):
    """record keys of shuffled handles with INT64_MIN, INT64_MAX and -1; the same keys already ascending need no pass; a record stream
    and two index streams of different ids mixed in one buffer"""
    rng = np.random.default_rng(51)
    hs = edge_handles(rng, 700)
    asc = MC.record_keys(41, hs)
    assert asc == sorted(asc)
    shuffled = [asc[i] for i in rng.permutation(len(asc))]
    mb, model, res = BG.run_case(ctx, [MC.sets(shuffled, 0, 38)], device=True, fixed=True)
    try:
        assert 0 < res["sort_passes"] <= 9 and [e[1] for e in mb.entries()] == asc  # one 64-bit image behind the 11 shared bytes: a single depth
    finally:
        mb.close()
    mb, model, res = BG.run_case(ctx, [MC.sets(asc[:300], 0, 38), MC.sets(asc[300:], 300, 38)], device=True, fixed=True)
    try:
        assert res["sort_passes"] == 0 and res["n_entries"] == len(asc)
        BG.commit_and_compare(ctx, mb, model, R.Store(), 7, 8)
    finally:
        mb.close()
    flip = lambda v: ((int(v) + (1 << 63)) & ((1 << 64) - 1)).to_bytes(8, "big")
    ix1 = [b"t" + flip(41) + b"_i" + flip(1) + b"\x03" + flip(int(h) % 97) + flip(h) for h in hs[:400]]            # BIGINT index, the handle in the key
    ix2 = [b"t" + flip(41) + b"_i" + flip(2) + b"\x01" + (b"s%06d\x00\x00" % (int(h) % 1000003))[:8] + b"\xf9" for h in hs[:400]]  # a unique string index
    pushes = [MC.sets(shuffled[:400], 0, 38), (MR.SET, ix1, [b"0"] * len(ix1)), (MR.SET, ix2, [flip(h) for h in hs[:400]]), MC.deletes(shuffled[100:150])]
    mb, model, res = BG.run_case(ctx, pushes, device=True)
    try:
        assert res["dels"] >= 1 and res["n_entries"] == len({k for _, ks, _ in pushes for k in ks})
        BG.commit_and_compare(ctx, mb, model, R.Store(), 9, 11)
    finally:
        mb.close()


def test_fuzz_against_the_model(ctx):
    pushes = MC.fuzz_pushes(np.random.default_rng(53), 20000)
    mb, model, res = BG.run_case(ctx, pushes, device=False)
    try:
        assert res["locks"] > 0 and res["dels"] > 0 and res["puts"] > 0 and res["n_entries"] < 6000
        BG.commit_and_compare(ctx, mb, model, R.Store(), 3, 4)
    finally:
        mb.close()


def test_get_hits_misses_deleted_and_out_of_range(ctx):
    pushes = [MC.sets([b"m1", b"m3", b"m5", b"m5\x00", b"m7"]), MC.deletes([b"m3"]), MC.locks([b"m9"])]
    mb, model, _ = BG.run_case(ctx, pushes)
    try:
        probes = [b"m1", b"m2", b"m3", b"m5", b"m5\x00", b"m5\x00\x00", b"m", b"\x00", b"zzzz", b"m9", b"m7"]
        kb, ko = BG.pack(probes)
        got = mb.get_packed(kb, ko, kb.size, len(probes)).tolist()
        keys = [e[1] for e in mb.entries()]
        assert got == [keys.index(p) if p in keys and p != b"m9" else -1 for p in probes] and got.count(-1) == 6  # (m9 is lock-only: a miss)
        assert mb.entries()[got[2]][0] == abi.MVCC_OP_DEL  # a deleted key is found, with Op_Del
        assert mb.Get(b"m1") == model.Get(b"m1") and mb.Get(b"m3") == b"" and mb.Get([b"m7", b"m5"]) == [model.Get(b"m7"), model.Get(b"m5")]
        for miss in (b"m2", b"m9"):
            with pytest.raises(kv.ErrNotExist):
                mb.Get(miss)
        # device probes through the fixed-length form
        from tinysql_amd.dupcheck import DevArray
        d = DevArray(ctx, np.frombuffer(b"m1m4m7", dtype=np.uint8).copy())
        try:
            assert mb.get_packed(d.p, None, 6, 3, device=True).tolist() == [keys.index(b"m1"), -1, keys.index(b"m7")]
        finally:
            d.free()
    finally:
        mb.close()


def test_get_before_finish_is_refused(ctx):
    h, out = C.c_void_p(), np.zeros(1, dtype=np.int64)
    _lib.check(ctx.lib.tsq_membuf_create(ctx.h, None, C.byref(h)), ctx.h)
    try:
        k = np.frombuffer(b"k", dtype=np.uint8).copy()
        assert ctx.lib.tsq_membuf_get(h, k.ctypes.data, None, 1, 1, 0, out.ctypes.data) == abi.ERR_INVALID and "not finished" in _lib.last_error(h)
        req = abi.MvccWriteReq()
        assert ctx.lib.tsq_membuf_request(h, C.byref(req)) == abi.ERR_INVALID
    finally:
        ctx.lib.tsq_membuf_destroy(h)


def test_both_limits(ctx):
    with kv.MemBuffer(ctx, entry_size_limit=500, total_size_limit=1000) as mb:
        with pytest.raises(_lib.TsqError, match="entry too large") as e:
            BG.push(mb, MR.SET, [b"x"], [bytes(500)])
        assert e.value.error_row == 0
        BG.push(mb, MR.SET, [b"x"], [bytes(499)])
        BG.push(mb, MR.SET, [b"y"], [bytes(499)])
        assert mb.finish()["size"] == 1000  # at the limit, not over it
        BG.push(mb, MR.DELETE, [b"z"])
        with pytest.raises(_lib.TsqError, match="transaction too large"):
            mb.finish()
        BG.push(mb, MR.DELETE, [b"y"])  # the final size counts: the delete of y takes 499 bytes out again
        assert mb.finish()["size"] == 500 + 1 + 1


REFUSALS = [("empty key", MR.SET, [b"a", b"b", b"", b"d", b""], [b"1", b"2", b"3", b"4", b"5"], 2),
            ("cannot set nil value", MR.SET, [b"a", b"b", b"c"], [b"1", b"", b""], 1),
            ("entry too large", MR.SET, [b"a", b"bb", b"c"], [bytes(9), bytes(9), bytes(10)], 1),
            ("empty key", MR.DELETE, [b""], None, 0),
            ("empty key", MR.LOCK, [b"l", b""], None, 1)]


@pytest.mark.parametrize("device", [False, True], ids=["host", "device"])
@pytest.mark.parametrize("message,kind,keys,values,row", REFUSALS, ids=["%s-%d" % (r[0].replace(" ", "_"), i) for i, r in enumerate(REFUSALS)])
def test_refused_pushes_name_the_row_and_add_nothing(ctx, message, kind, keys, values, row, device):
    before = [MC.sets([b"k2", b"k1"], 0, 3), MC.locks([b"k3"])]
    with kv.MemBuffer(ctx, entry_size_limit=10) as mb:
        BG.fill(mb, before, device)
        with pytest.raises(_lib.TsqError, match=message) as e:
            BG.push(mb, kind, keys, values, device)
        assert e.value.status == abi.ERR_INVALID and e.value.error_row == row == MR.first_refused_row(kind, keys, values, 10)
        BG.check_finished(mb, MR.replay(before))  # the buffer is as it was
        after = [MC.sets([b"k0"], 3, 3)]
        BG.fill(mb, after, device)  # ... and takes the next push behind the entries it had
        BG.check_finished(mb, MR.replay(before + after))


def test_bad_offsets_and_arguments_are_refused(ctx):
    with kv.MemBuffer(ctx) as mb:
        kb = np.frombuffer(b"abcdef", dtype=np.uint8).copy()
        for offs, row in (([0, 3, 2, 6], 1), ([0, 3, 7, 7], 1), ([-1, 3, 6, 6], 0)):
            with pytest.raises(_lib.TsqError, match="offsets decrease or leave their buffer") as e:
                mb.push_packed(MR.DELETE, kb, np.array(offs, dtype=np.int64), 6, 3)
            assert e.value.error_row == row
        with pytest.raises(_lib.TsqError, match="multiple of n"):
            mb.push_packed(MR.DELETE, kb, None, 6, 4)
        with pytest.raises(_lib.TsqError, match="kind"):
            mb.push_packed(3, kb, None, 6, 3)
        assert mb.finish()["n_entries"] == 0 and mb.finish()["primary_index"] == -1 and mb.entries() == []


def test_second_finish_after_more_pushes(ctx):
    first = [MC.sets([b"b", b"a", b"c"]), MC.locks([b"d"])]
    more = [MC.deletes([b"a"]), MC.sets([b"d", b"0"], 10), MC.locks([b"c", b"e"])]
    with kv.MemBuffer(ctx) as mb:
        BG.fill(mb, first)
        BG.check_finished(mb, MR.replay(first))
        BG.fill(mb, more, device=True)
        got = BG.check_finished(mb, MR.replay(first + more))  # what one finish over all pushes gives
        assert got == {**mb.finish(), "kernel_ms": got["kernel_ms"]}  # and a third finish with nothing new the same again


def test_host_conveniences_batch_until_finish(ctx):
    with kv.MemBuffer(ctx) as mb:
        model = MR.Model()
        for f in (lambda b: b.Set(b"k1", b"v1"), lambda b: b.Set(b"k0", b"v0"), lambda b: b.Delete(b"k1"), lambda b: b.LockKeys(b"k2", b"k0"),
                  lambda b: b.Set(b"k2", b"v2"), lambda b: b.Delete(b"k9")):
            f(mb)
            f(model)
        BG.check_finished(mb, model)
        assert mb.Get(b"k2") == b"v2" and mb.Get(b"k9") == b""
        mb.Set(b"nil", b"")
        mb.Delete(b"k0")
        with pytest.raises(_lib.TsqError, match="cannot set nil value"):
            mb.finish()
        model.Delete(b"k0")  # the refused Set is dropped, the entry queued behind it stays and goes in with the next finish
        BG.check_finished(mb, model)


def test_request_on_a_store_with_history_and_a_foreign_lock(ctx):
    """the buffer's request over a store that holds versions and a foreign lock: ErrLocked names the key, nothing is written; after the
    lock's transaction is rolled back the same buffer commits"""
    s = W.writable_random_store(np.random.default_rng(57), 0)
    s.put(b"k-b", b"old", 1, 2)
    s.prewrite([(R.OP_PUT, b"k-d", b"theirs")], b"k-d", 4)
    pushes = dict(MC.order_cases())["orders_one_buffer"]
    mb, model, _ = BG.run_case(ctx, pushes)
    ms = WG.open_rw(ctx, s)
    try:
        with pytest.raises(M.ErrLocked) as e:
            M.write_membuffer(ms, mb, 10, 20)
        assert e.value.RawKey == b"k-d" and e.value.StartTS == 4
        WG.compare_store(ms, s)
    finally:
        ms.close()
    W.rollback(s, [b"k-d"], 4)
    BG.commit_and_compare(ctx, mb, model, s, 10, 20)
    mb.close()
