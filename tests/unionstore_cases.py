"""Shared by the CPU and the GPU tests of the union store: the stores, buffers and reads of the edge grid, the hand-built store of the
lock outcomes, and the fuzz inputs.  A case is (name, mvcc_ref.Store, pushes or None, ranges, points); the expectation is always
tests/unionstore_ref.py's."""
import json
import os

import numpy as np

from tests import membuf_cases as MC
from tests import membuf_ref as MB
from tests import mvcc_ref as R
from tests import unionstore_ref as U

BLOCK = 256  # candidates per workgroup of the merged route's kernels (tsq_unionstore.hip): the sizes around it are the size grid's
LIMITS = lambda n: [-1, 0, 1, 2, 64, n - 1, n, n + 1]
ALPHABET = (0x00, 0x61, 0x62)


def golden():
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "unionstore_cases.json")) as f:
        return json.load(f)["cases"]


def store_of(pairs, locks=(), commit_ts=10):
    """a store with one PUT version per pair at commit_ts, and the locks given as (key, Lock)"""
    s = R.Store()
    for k, v in pairs:
        s.versions[k] = [R.Value(R.PUT, commit_ts - 1, commit_ts, v)]
    for k, l in locks:
        s.locks[k] = l
    return s


def val(k, tag=b"s"):
    return tag + b":" + k[:6] + b"." * (len(k) % 5)


def bounds_for(keys):
    """ranges that begin or end on each of the keys given, just behind it, on a proper prefix of it, and the open bounds"""
    ks = sorted(set(keys))
    rs = [(b"", b""), (ks[0], ks[-1]), (ks[-1], ks[0]), (ks[0], ks[0])]
    for k in ks[::max(1, len(ks) // 10)] + ks[-1:]:
        rs += [(k, b""), (b"", k), (k + b"\x00", b""), (b"", k + b"\x00"), (k[:-1], k + b"\x00"), (k, R.prefix_next(k))]
    rs += [(ks[0], ks[len(ks) // 2] + b"\x00"), (ks[len(ks) // 3], b""), (ks[len(ks) // 3], b"")]  # overlapping, identical
    return rs


def edge_cases():
    rng = np.random.default_rng(61)
    out = []
    sk = [b"k%02d" % i for i in range(0, 40, 2)]
    store = store_of([(k, val(k)) for k in sk])
    inter = [b"k%02d" % i for i in range(1, 40, 2)]
    pts = lambda ks: list(ks)[:12] + [b"", b"zz", b"k0", list(ks)[0], list(ks)[0]] if ks else [b"a", b""]

    def add(name, st, pushes, keys):
        out.append((name, st, pushes, bounds_for(keys) if keys else [(b"", b""), (b"a", b"")], pts(keys)))
    add("empty_buffer", store, [], sk)
    add("no_buffer", store, None, sk)
    add("empty_store", R.Store(), [MC.sets(inter, 0, 5), MC.deletes(inter[::3])], inter)
    add("both_empty", R.Store(), [], [])
    add("neither", R.Store(), None, [])
    add("buffer_before", store, [MC.sets([b"a%d" % i for i in range(9)], 0, 4), MC.deletes([b"a3"])], sk + [b"a0", b"a8"])
    add("buffer_after", store, [MC.sets([b"z%d" % i for i in range(9)], 0, 4), MC.deletes([b"z3"])], sk + [b"z0", b"z8"])
    add("interleaved", store, [MC.sets(inter, 0, 7), MC.deletes(inter[::4])], sk + inter)
    add("all_equal_put", store, [MC.sets(sk, 0, 9)], sk)
    add("all_equal_del", store, [MC.deletes(sk)], sk)
    add("dangling_del", store, [MC.deletes([b"k01", b"k39", b"a", b"zz"]), MC.sets([b"k05"], 0, 3)], sk + [b"k01", b"a"])
    add("lock_only_does_not_shadow", store, [MC.locks([b"k04", b"k05", b"k10"]), MC.sets([b"k06"], 0, 3), MC.deletes([b"k08"])], sk + [b"k05"])
    # a store key whose visible version is a delete, or only rollbacks, under a buffer PUT (and beside one that is simply not there)
    inv = store_of([(k, val(k)) for k in sk])
    inv.versions[b"k04"] = [R.Value(R.DELETE, 8, 9, b""), R.Value(R.PUT, 3, 4, b"old")]
    inv.versions[b"k08"] = [R.Value(R.ROLLBACK, 7, 7, b""), R.Value(R.ROLLBACK, 5, 5, b"")]
    inv.versions[b"k12"] = [R.Value(R.PUT, 50, 51, b"later")]  # (not visible at the tests' read timestamp of 20)
    add("invisible_under_put", inv, [MC.sets([b"k04", b"k08", b"k12", b"k16"], 0, 6), MC.deletes([b"k06"])], sk)
    # key lengths 1, 7, 8, 9, 16, 17, 19: one a prefix of the other, and pairs that differ only in the last byte
    stem = bytes(rng.integers(1, 255, 19, dtype=np.uint8))
    lens = (1, 7, 8, 9, 16, 17, 19)
    pref = [stem[:n] for n in lens]
    last = [stem[:n - 1] + bytes([stem[n - 1] ^ 1]) for n in lens]
    add("lengths_prefixes", store_of([(k, val(k)) for k in pref[::2] + last[1::2]]), [MC.sets(pref[1::2] + last[::2], 0, 5), MC.deletes([pref[2]]), MC.sets([last[1]], 9, 4)],
        pref + last)
    return out


def sized(n_store, n_buf, overlap_every=3, seed=0):
    """n_store store keys and n_buf buffer keys of 8 bytes; every overlap_every-th buffer key is a store key (a PUT or a DEL)"""
    rng = np.random.default_rng(1000 + seed)
    pool = sorted({bytes(rng.integers(97, 100, 8, dtype=np.uint8)) for _ in range(4 * (n_store + n_buf) + 16)})
    assert len(pool) >= n_store + n_buf
    pick = rng.permutation(len(pool))
    sk = sorted(pool[i] for i in pick[:n_store])
    fresh = [pool[i] for i in pick[n_store:n_store + n_buf]]
    bk = [sk[(7 * i) % n_store] if n_store and i % overlap_every == 0 else fresh[i] for i in range(n_buf)]
    bk = list(dict.fromkeys(bk))
    while len(bk) < n_buf:  # (the overlap repeated a store key)
        bk.append(fresh[len(bk)])
    store = store_of([(k, val(k)) for k in sk])
    pushes = [MC.sets(bk[::2] + bk[1::4], 0, 6), MC.deletes(bk[3::4])] if bk else []
    return store, pushes


def size_grid():
    """(name, store, pushes): merged candidate counts of BLOCK - 1, BLOCK, BLOCK + 1 and 2 BLOCK + 1; 63 / 64 / 65 entries on either
    side; one entry against 3 BLOCK"""
    out = []
    for c in (BLOCK - 1, BLOCK, BLOCK + 1, 2 * BLOCK + 1):
        out.append(("candidates_%d" % c, ) + sized(c // 2, c - c // 2, seed=c))
    for n in (63, 64, 65):
        out.append(("store_%d" % n, ) + sized(n, 100, seed=n))
        out.append(("buffer_%d" % n, ) + sized(100, n, seed=100 + n))
    out.append(("one_store_key", ) + sized(1, 3 * BLOCK, overlap_every=1, seed=7))
    out.append(("one_buffer_key", ) + sized(3 * BLOCK, 1, overlap_every=1, seed=8))
    return out


READ_TS = 20


def lock_store():
    """the hand-built store of the lock outcomes: 60 keys k00 .. k59 committed at 10; locks (all of other transactions, start_ts 15,
    read at 20) on k10 (the buffer PUTs it), k20 (the buffer DELs it), k30 (untouched), k40 (its predecessor k39 is shadowed by a PUT),
    k50 (its predecessor k49 is DELeted); a lock-only buffer key on k05.  -> (store, pushes)"""
    sk = [b"k%02d" % i for i in range(60)]
    mk = lambda k: R.Lock(15, b"prim-" + k, b"x", R.OP_PUT, 33)
    store = store_of([(k, val(k)) for k in sk], [(k, mk(k)) for k in (b"k10", b"k20", b"k30", b"k40", b"k50")])
    pushes = [MC.sets([b"k10", b"k39", b"k03", b"k25x"], 0, 5), MC.deletes([b"k20", b"k49", b"k07"]), MC.locks([b"k05"])]
    return store, pushes


def lock_reads():
    """[(ranges, desc, limit)] over lock_store(): every outcome of the lock rule, in both directions"""
    out = []
    for lo, hi in ((b"k00", b"k12"), (b"k12", b"k22"), (b"k22", b"k32"), (b"k32", b"k42"), (b"k42", b"k52"), (b"k52", b""), (b"k05", b"k10"), (b"k10", b"k11"),
                   (b"k11", b"k20"), (b"k39", b"k41"), (b"k49", b"k51")):
        for desc in (False, True):
            for limit in (-1, 0, 1, 2, 3, 7, 8, 9, 10, 11):
                out.append(([(lo, hi)], desc, limit))
    out += [([(b"k00", b"k05"), (b"k06", b"k09"), (b"k08", b"k12")], d, l) for d in (False, True) for l in (-1, 4, 5, 6, 7, 8, 9, 10)]
    return out


def lock_points():
    return [[b"k00", b"k03", b"k07", b"k20", b"k05", b"k25x", b"nokey"], [b"k00", b"k20", b"k10"], [b"k01", b"k30", b"k20"], [b"k20", b"k20", b"k40"], [b"k02", b"k50"]]


def fuzz_keys(rng, n, max_len=12):
    out = set()
    letters = np.array(ALPHABET, dtype=np.uint8)
    while len(out) < n:
        lens = rng.integers(1, max_len + 1, n)
        mat = letters[rng.integers(0, len(letters), (n, max_len))]
        out.update(mat[i, :lens[i]].tobytes() for i in range(n))
    return sorted(out)[:n] if len(out) > n else sorted(out)


def fuzz_store(rng, n_keys, n_locks, max_len=12):
    """n_keys keys over the three-letter alphabet with 1..3 versions (puts, deletes, rollbacks) committed below 100; n_locks locks of other
    transactions with start_ts 150 on stored keys: a read at 120 ignores them, a read at 200 meets them"""
    keys = fuzz_keys(rng, n_keys, max_len)
    s = R.Store()
    kinds = rng.integers(0, 10, len(keys))
    for k, kind in zip(keys, kinds):
        if kind < 7:
            s.versions[k] = [R.Value(R.PUT, 49, 50, b"v" + k[:5])]
        elif kind == 7:
            s.versions[k] = [R.Value(R.DELETE, 59, 60, b""), R.Value(R.PUT, 49, 50, b"old")]
        elif kind == 8:
            s.versions[k] = [R.Value(R.ROLLBACK, 70, 70, b""), R.Value(R.PUT, 49, 50, b"w" + k[:3])]
        else:
            s.versions[k] = [R.Value(R.ROLLBACK, 70, 70, b"")]
    for i in rng.choice(len(keys), n_locks, replace=False):
        s.locks[keys[i]] = R.Lock(150, b"p" + keys[i][:3], b"x", int(rng.choice([R.OP_PUT, R.OP_DEL])), 9)
    return s


def fuzz_pushes(rng, store, n_entries, max_len=12):
    """n_entries buffer writes: a third on stored keys (locked ones among them), the rest drawn like the store's keys — so many
    coincide; PUTs, DELs and lock-only keys"""
    sk = store.keys()
    lk = sorted(store.locks)
    keys = [sk[int(i)] for i in rng.integers(0, len(sk), n_entries // 3)] + lk + fuzz_keys(rng, n_entries - n_entries // 3, max_len)
    order = rng.permutation(len(keys))
    keys = [keys[i] for i in order]
    a, b = int(len(keys) * 0.6), int(len(keys) * 0.9)
    return [MC.sets(keys[:a], 0, 6), MC.deletes(keys[a:b]), MC.locks(keys[b:]), MC.sets(keys[b::7], 5, 3)]


def fuzz_ranges(rng, store, dirty, n, span=200):
    ks = sorted(set(store.keys()) | set(dirty.all_keys))
    out = []
    for _ in range(n):
        i = int(rng.integers(0, len(ks)))
        j = min(len(ks) - 1, max(0, i + int(rng.integers(-20, span))))
        a, b = ks[i], ks[j]
        w = rng.random()
        if w < 0.2:
            a = a[:max(1, len(a) - int(rng.integers(0, 3)))] if len(a) > 6 else a  # (a proper prefix; a short one would span the whole store)
        elif w < 0.4:
            b = b + bytes(rng.choice(ALPHABET, int(rng.integers(1, 3))).astype(np.uint8))
        out.append((a, b))
    return out


def fuzz_points(rng, store, dirty, n):
    sk, bk = store.keys(), dirty.all_keys
    lk = sorted(store.locks)
    out = [sk[int(i)] for i in rng.integers(0, len(sk), n // 3)] + [bk[int(i)] for i in rng.integers(0, len(bk), n // 3)]
    out += fuzz_keys(rng, n - len(out) - 2, 9) + [b"", out[0]]
    return [out[i] for i in rng.permutation(len(out))], lk


def model_of(pushes):
    return None if pushes is None else MB.replay(pushes)


def answer(store, dirty, ranges, ts, desc, limit):
    """the model's answer in the comparable form of both tests: ("ok", pairs, from_buffer, range_counts) or ("locked", raw key, n_pairs)"""
    try:
        got = U.read(store, dirty, ranges, ts, desc, limit)
        return ("ok", got["pairs"], got["from_buffer"], got["range_counts"])
    except U.Locked as e:
        return ("locked", e.err.RawKey, e.n_pairs)


def point_answer(store, dirty, keys, ts):
    try:
        return ("ok", U.get(store, dirty, keys, ts))
    except U.Locked as e:
        return ("locked", e.err.RawKey, e.n_pairs)
