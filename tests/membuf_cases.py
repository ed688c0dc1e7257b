"""The inputs the CPU test (the host build of tsq_membuf_dp.h) and the GPU test (tsq_membuf_*) of the transaction buffer share: named
lists of pushes [(kind, keys, values or None)], each answered by tests/membuf_ref.Model.  Values are derived from the key and the
sequence number, so that "the last write wins" shows in the bytes."""
import numpy as np

from tests import membuf_ref as MR

TILE = 4096  # entries per tile of a radix pass (TSQ_MB_T of tsq_membuf.hip)
KEY_LENS = (1, 7, 8, 9, 15, 16, 17, 19, 63, 64, 65, 300)
VALUE_LENS = (1, 63, 64, 65, 300)
COUNTS = (0, 1, 2, 63, 64, 65, 255, 256, 257, 2 * TILE + 1)


def value_for(key, seq, length):
    seed = (b"%d:" % seq) + key[:8]
    return (seed * (length // len(seed) + 1))[:length]


def sets(keys, seq0=0, vlen=None):
    return (MR.SET, list(keys), [value_for(k, seq0 + i, vlen if vlen else VALUE_LENS[(seq0 + i) % len(VALUE_LENS)]) for i, k in enumerate(keys)])


def deletes(keys):
    return (MR.DELETE, list(keys), None)


def locks(keys):
    return (MR.LOCK, list(keys), None)


def random_keys(rng, n, length, shared=0):
    """n distinct keys of `length` bytes that share their first `shared` bytes"""
    head = bytes(rng.integers(0, 256, shared, dtype=np.uint8))
    out = set()
    while len(out) < n:
        out.add(head + bytes(rng.integers(0, 256, length - shared, dtype=np.uint8)))
    out = list(out)
    rng.shuffle(out)
    return out


def key_set_cases():
    """the key sets of the issue's grid, each as one shuffled push of Sets"""
    rng = np.random.default_rng(41)
    cases = []
    # keys that differ only in trailing 0x00 bytes — behind shared prefixes that end inside, at and across an 8-byte window edge
    for stem in (b"ab", b"abcdefg", b"abcdefgh", b"abcdefghi", b"0123456789abcdef"):
        ks = [stem + b"\x00" * z for z in range(0, 12)]
        rng.shuffle(ks)
        cases.append(("trailing_zeros_%d" % len(stem), [sets(ks)]))
    # proper prefixes of others at and across window edges behind a shared prefix of 11 bytes (a record-key prefix)
    pre = b"t\x80\x00\x00\x00\x00\x00\x00\x29_r"
    body = bytes(range(1, 40))
    ks = [pre + body[:l] for l in (1, 7, 8, 9, 15, 16, 17, 24, 25, 39)] + [pre + body[:8] + b"\x00", pre + body[:16] + b"\x00\x00", pre + body[:8] + b"\x00\x01"]
    rng.shuffle(ks)
    cases.append(("proper_prefixes", [sets(ks)]))
    # no shared prefix at all: every first byte differs
    ks = [bytes([b]) + bytes(rng.integers(0, 256, int(rng.integers(0, 20)), dtype=np.uint8)) for b in rng.permutation(256)]
    cases.append(("no_shared_prefix", [sets(ks)]))
    # everything shared but the last byte, for every key length of the grid
    for length in KEY_LENS:
        head = bytes(rng.integers(0, 256, length - 1, dtype=np.uint8))
        ks = [head + bytes([b]) for b in rng.permutation(256)[:200]]
        cases.append(("last_byte_len%d" % length, [sets(ks)]))
    # every key length of the grid in one buffer, random bodies, every value length
    ks = [k for length in KEY_LENS for k in random_keys(rng, 5, length)]
    rng.shuffle(ks)
    cases.append(("mixed_lengths", [sets(ks)]))
    # all n keys equal: one survivor, the last
    for n in (2, 65, 300):
        cases.append(("all_equal_%d" % n, [sets([b"same-key"] * n)]))
    return cases


def order_cases():
    """set→delete, delete→set, lock→set, set→lock, lock alone, a duplicate lock — each in one buffer through single pushes (`one`: one
    push per kind run) and across pushes with other keys around them"""
    a, b, c, d, e, f = b"k-a", b"k-b", b"k-c", b"k-d", b"k-e", b"k-f"
    other = [b"k-0", b"k-zz", b"j", b"k-c\x00"]
    cases = []
    cases.append(("orders_one_buffer", [sets([a]), deletes([a]), deletes([b]), sets([b], 7), locks([c]), sets([c], 9), sets([d], 11), locks([d]), locks([e]),
                                        locks([f]), locks([f])]))
    cases.append(("orders_across_pushes", [sets(other[:2] + [a, d]), locks([c, e, f]), deletes([a, b] + other[2:3]), sets([b, c] + other[3:], 20),
                                           locks([d, f, other[0]])]))
    cases.append(("lock_only", [locks([b"q", b"p", b"q", b"r"])]))  # primary: the first lock pushed, "q" — not the smallest
    cases.append(("lock_then_smaller_put", [locks([b"a"]), sets([b"m"]), deletes([b"z"])]))  # primary: "m", the smallest non-lock key
    cases.append(("set_delete_set_same_push", [(MR.SET, [a, a, b, a], [b"1", b"22", b"333", b"4444"])]))
    return cases


def record_keys(table_id, handles):
    """tablecodec.EncodeRowKeyWithHandle: 't' + the table id + '_r' + the handle, both ints sign-flipped big-endian (19 bytes)"""
    flip = lambda v: ((int(v) + (1 << 63)) & ((1 << 64) - 1)).to_bytes(8, "big")
    return [b"t" + flip(table_id) + b"_r" + flip(h) for h in handles]


def count_cases():
    """every count of the grid: record keys of shuffled handles with a tenth of them written twice"""
    rng = np.random.default_rng(43)
    cases = []
    for n in COUNTS:
        hs = rng.choice(np.arange(-5 * max(n, 1), 5 * max(n, 1)), n, replace=False)
        ks = record_keys(41, hs)
        again = ks[: n // 10]
        cases.append(("count_%d" % n, [sets(ks, 0, 38)] + ([sets(again, n, 38)] if again else [])))
    return cases


def fuzz_pushes(rng, n, alphabet=(0x00, 0x61, 0x62), max_len=40, n_distinct=None):
    """n entries in pushes of random kinds and sizes: keys over a 3-letter alphabet that includes 0x00, lengths 1..max_len, drawn from a
    pool a quarter the size so that most keys are written several times"""
    pool_n = n_distinct or max(n // 4, 1)
    pool = [bytes(rng.choice(alphabet, int(rng.integers(1, max_len + 1))).astype(np.uint8)) for _ in range(pool_n)]
    pushes, seq = [], 0
    while seq < n:
        m = int(min(n - seq, rng.integers(1, max(2, n // 7))))
        ks = [pool[int(i)] for i in rng.integers(0, pool_n, m)]
        kind = int(rng.choice([MR.SET, MR.SET, MR.DELETE, MR.LOCK]))
        pushes.append(sets(ks, seq) if kind == MR.SET else (kind, ks, None))
        seq += m
    return pushes


def all_small_cases():
    return key_set_cases() + order_cases() + count_cases()
