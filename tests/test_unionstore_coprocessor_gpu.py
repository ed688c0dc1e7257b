"""GPU: the duplicate-key checker's stores built from a transaction's merged read — coprocessor.DeviceTable.from_pairs / from_union and
DeviceIndex.from_union over a kv.UnionStore — against the same stores built by the existing host constructors from the model's merged
pairs (tests/unionstore_ref.py): the handles, the stored rows and their offsets, the distinct index entries.  A table built from the
committed rows alone differs: it lacks the rows the transaction inserted and still holds the ones it deleted."""
import numpy as np
import pytest

from tests import membuf_cases as MC
from tests import membuf_gpu_helpers as BG
from tests import memread_ref as MRD
from tests import unionstore_cases as K
from tests import unionstore_gpu_helpers as UG
from tests import unionstore_ref as U
from tinysql_amd import _lib
from tinysql_amd import coprocessor as CP

pytestmark = pytest.mark.gpu

TID, IDX = 41, 2
be = lambda h: (int(h) & ((1 << 64) - 1)).to_bytes(8, "big")


def index_key(a):
    return MRD.index_prefix(TID, IDX) + b"\x03" + MRD.flip(a)


def world():
    """500 committed rows (handles 0 .. 499, a = 10 h) with their unique-index entries; the transaction inserts 300 rows, rewrites 20 and
    deletes 50 — record keys and index entries alike; another table's and another index's keys lie around them"""
    hs = list(range(500))
    rec = MC.record_keys(TID, hs)
    pairs = [(k, b"row-%d" % h + b"." * (h % 7)) for k, h in zip(rec, hs)] + [(index_key(10 * h), be(h)) for h in hs]
    pairs += [(k, b"other") for k in MC.record_keys(TID + 1, [1, 2])] + [(MRD.index_prefix(TID, IDX + 1) + b"\x03" + MRD.flip(5), be(5))]
    store = K.store_of(sorted(pairs))
    new = list(range(1000, 1300))
    gone = hs[100:150]
    pushes = [(0, MC.record_keys(TID, new), [b"new-%d" % h for h in new]), (0, [index_key(10 * h) for h in new], [be(h) for h in new]),
              (0, MC.record_keys(TID, hs[:20]), [b"rewritten-%d" % h for h in hs[:20]]),
              MC.deletes(MC.record_keys(TID, gone) + [index_key(10 * h) for h in gone]), MC.deletes(MC.record_keys(TID, [7000])),
              (0, [index_key(10 * 2000 + 1)], [b"0"])]  # (an entry with a NULL cell: not distinct, not in the checker's index)
    return store, pushes, sorted(set(hs) - set(gone) | set(new))


def table_contents(ctx, t):
    hs = np.zeros(max(t.n, 1), np.int64)
    offs = np.zeros(t.n + 1, np.int64)
    ctx.d2h(offs, t.do.p)
    vals = np.zeros(max(t.n_bytes, 1), np.uint8)
    if t.n:
        ctx.d2h(hs[:t.n], t.dh)
        ctx.d2h(vals[:t.n_bytes], t.dv.p)
    return hs[:t.n].tolist(), offs.tolist(), vals[:t.n_bytes].tobytes()


def index_contents(ctx, ix):
    ko, hs, kb = np.zeros(ix.n + 1, np.int64), np.zeros(max(ix.n, 1), np.int64), np.zeros(max(ix.key_bytes, 1), np.uint8)
    ctx.d2h(ko, ix.key_offsets.p)
    if ix.n:
        ctx.d2h(hs[:ix.n], ix.handles.p)
        ctx.d2h(kb[:ix.key_bytes], ix.keys.p)
    return ix.n, ko.tolist(), hs[:ix.n].tolist(), kb[:ix.key_bytes].tobytes()


def test_device_table_and_index_from_the_union_read(ctx):
    store, pushes, want_handles = world()
    with UG.Opened(ctx, store, pushes) as o:
        lo, hi = MRD.record_prefix(TID), MRD.record_prefix(TID)[:-1] + b"s"
        merged = U.read(store, o.dirty, [(lo, hi)], o.ts)["pairs"]
        assert [MRD.signed(int.from_bytes(k[11:], "big") ^ (1 << 63)) for k, _ in merged] == want_handles
        vb, vo = BG.pack([v for _, v in merged])
        by_host = CP.DeviceTable(ctx, b"".join(k for k, _ in merged), vb, vo)
        by_union = CP.DeviceTable.from_union(o.us, TID)
        committed = o.ms.scan([(lo, hi)], o.ts)
        by_pairs = CP.DeviceTable.from_pairs(ctx, committed)  # (takes the pairs over)
        try:
            assert table_contents(ctx, by_union) == table_contents(ctx, by_host) and by_union.n == len(want_handles) == 750
            got = table_contents(ctx, by_pairs)
            assert got[0] == list(range(500)) and got != table_contents(ctx, by_host)  # the committed rows alone: what the checker saw before
        finally:
            by_host.close()
            by_union.close()
            by_pairs.close()
        ipre = MRD.index_prefix(TID, IDX)
        imerged = U.read(store, o.dirty, [(ipre, MRD.prefix_next(ipre))], o.ts)["pairs"]
        kb, ko = BG.pack([k for k, _ in imerged])
        vb, vo = BG.pack([v for _, v in imerged])
        ix_host = CP.DeviceIndex(ctx, kb, ko, vb, vo)
        ix_union = CP.DeviceIndex.from_union(o.us, TID, IDX)
        try:
            assert index_contents(ctx, ix_union) == index_contents(ctx, ix_host) and ix_union.n == 750 and len(imerged) == 751
        finally:
            ix_host.close()
            ix_union.close()


def test_from_pairs_refuses_keys_that_are_not_record_keys(ctx):
    store, pushes, _ = world()
    with UG.Opened(ctx, store, pushes) as o:
        with pytest.raises(_lib.TsqError):
            CP.DeviceTable.from_pairs(ctx, o.us.scan([(MRD.index_prefix(TID, IDX), b"")]))
        empty = CP.DeviceTable.from_union(o.us, TID + 5)
        assert empty.n == 0
        empty.close()
