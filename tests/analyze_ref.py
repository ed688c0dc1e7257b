"""Pure Python / numpy restatement of what an ANALYZE TABLE computes per column and per sorted stream (DESIGN.md "ANALYZE"): the datum
bytes of a value, murmur3 x64_128, the FM sketch (sequential as the reference inserts, and the canonical form the GPU returns), the CM
sketch, the sampler and SortedBuilder (row by row, and the run-jump form the walk kernel takes).  The GPU tests compare exactly with
this module; tests/test_analyze_cpu.py pins it on published vectors and on the reference's own test values."""
import struct

import numpy as np

M64 = (1 << 64) - 1
I64, U64, F32, F64, BYTES = 0, 1, 2, 3, 4


# ---------------------------------------------------------------- datum bytes (util/codec/codec.go:74-109)
def uvarint(x):
    out = bytearray()
    while x >= 0x80:
        out.append((x & 0x7f) | 0x80)
        x >>= 7
    out.append(x)
    return bytes(out)


def varint(v):
    return uvarint(((v << 1) ^ (v >> 63)) & M64)


def mem_bytes(b):
    """EncodeBytes (util/codec/bytes.go:35-67): groups of 8 bytes, each followed by 0xFF - pad count"""
    out = bytearray()
    for g in range(len(b) // 8 + 1):
        part = b[8 * g:8 * g + 8]
        pad = 8 - len(part)
        out += part + b"\0" * pad
        out.append(0xFF - pad)
    return bytes(out)


def encode_datum(tp, v, comparable=False):
    if v is None:
        return b"\x00"
    if tp in (F32, F64):
        f = float(np.float32(v)) if tp == F32 else float(v)
        bits = struct.unpack("<Q", struct.pack("<d", f))[0]
        u = (bits | (1 << 63)) if f >= 0 else (~bits & M64)
        return b"\x05" + struct.pack(">Q", u)
    if tp == BYTES:
        b = bytes(v)
        return b"\x01" + mem_bytes(b) if comparable else b"\x02" + varint(len(b)) + b
    v = int(v)
    if comparable:
        return b"\x03" + struct.pack(">Q", (v & M64) ^ (1 << 63)) if tp == I64 else b"\x04" + struct.pack(">Q", v & M64)
    return b"\x08" + varint(v) if tp == I64 else b"\x09" + uvarint(v & M64)


def wrap_bytes(e):
    """the bytes datum of an encoded value, as FMSketch.InsertValue hashes it on the storage side"""
    return b"\x02" + varint(len(e)) + e


# ---------------------------------------------------------------- murmur3 x64_128, seed 0
C1, C2 = 0x87c37b91114253d5, 0x4cf5ad432745937f


def _rotl(x, r):
    return ((x << r) | (x >> (64 - r))) & M64


def _fmix(k):
    k ^= k >> 33
    k = (k * 0xff51afd7ed558ccd) & M64
    k ^= k >> 33
    k = (k * 0xc4ceb9fe1a85ec53) & M64
    k ^= k >> 33
    return k


def murmur3_128(data, seed=0):
    data = bytes(data)
    n = len(data)
    h1 = h2 = seed
    nblocks = n // 16
    for i in range(nblocks):
        k1, k2 = struct.unpack_from("<QQ", data, 16 * i)
        k1 = (k1 * C1) & M64
        k1 = _rotl(k1, 31)
        k1 = (k1 * C2) & M64
        h1 ^= k1
        h1 = _rotl(h1, 27)
        h1 = (h1 + h2) & M64
        h1 = (h1 * 5 + 0x52dce729) & M64
        k2 = (k2 * C2) & M64
        k2 = _rotl(k2, 33)
        k2 = (k2 * C1) & M64
        h2 ^= k2
        h2 = _rotl(h2, 31)
        h2 = (h2 + h1) & M64
        h2 = (h2 * 5 + 0x38495ab5) & M64
    tail = data[16 * nblocks:]
    k1 = int.from_bytes(tail[:8], "little")
    k2 = int.from_bytes(tail[8:], "little")
    if len(tail) > 8:
        k2 = (k2 * C2) & M64
        k2 = _rotl(k2, 33)
        k2 = (k2 * C1) & M64
        h2 ^= k2
    if len(tail) > 0:
        k1 = (k1 * C1) & M64
        k1 = _rotl(k1, 31)
        k1 = (k1 * C2) & M64
        h1 ^= k1
    h1 ^= n
    h2 ^= n
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    h1 = _fmix(h1)
    h2 = _fmix(h2)
    h1 = (h1 + h2) & M64
    h2 = (h2 + h1) & M64
    return h1, h2


def murmur3_64(data):
    return murmur3_128(data)[0]


# ---------------------------------------------------------------- FM sketch (statistics/fmsketch.go:49-62)
def fm_sequential(hashes, max_size):
    """insertHashValue one after the other -> (mask, set)"""
    mask, hs = 0, set()
    for h in hashes:
        if h & mask != 0:
            continue
        hs.add(h)
        if len(hs) > max_size:
            mask = mask * 2 + 1
            hs = {x for x in hs if x & mask == 0}
    return mask, hs


def fm_canonical(hashes, max_size):
    """mask = 2^k - 1 for the smallest k at which the distinct hashes with h & mask == 0 number at most max_size; the set is those"""
    hs = set(hashes)
    mask = 0
    while True:
        keep = {x for x in hs if x & mask == 0}
        if len(keep) <= max_size:
            return mask, keep
        hs = keep
        mask = mask * 2 + 1


def fm_merge(a, b, max_size):
    """two canonical sketches (mask, set) of one max_size -> the canonical sketch of the union of their inputs"""
    mask = max(a[0], b[0])
    m, keep = fm_canonical([h for h in a[1] | b[1] if h & mask == 0], max_size)
    return max(mask, m), {h for h in keep if h & max(mask, m) == 0}


def fm_ndv(sk):
    return (sk[0] + 1) * len(sk[1])


# ---------------------------------------------------------------- CM sketch
def cm_sketch(cells, depth, width):
    """cells: the byte strings of the non-NULL cells -> uint32[depth, width]; counter (h1 + h2 * i) mod width of row i"""
    t = np.zeros((depth, width), dtype=np.uint32)
    for e in cells:
        h1, h2 = murmur3_128(e)
        for i in range(depth):
            t[i, ((h1 + h2 * i) & M64) % width] += np.uint32(1)
    return t


def cm_sketch_hashed(h1, h2, depth, width):
    """the same from arrays of hash pairs (uint64)"""
    t = np.zeros((depth, width), dtype=np.uint32)
    h1 = np.asarray(h1, dtype=np.uint64)
    h2 = np.asarray(h2, dtype=np.uint64)
    for i in range(depth):
        with np.errstate(over="ignore"):
            idx = (h1 + h2 * np.uint64(i)) % np.uint64(width)
        t[i] = np.bincount(idx.astype(np.int64), minlength=width).astype(np.uint32)
    return t


# ---------------------------------------------------------------- the sampler
def splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


def sample_ordinals(notnull, seed, max_sample_size):
    """notnull[r] for every pushed row -> the ordinals of the sample, ascending"""
    rows = [r for r, nn in enumerate(notnull) if nn]
    rows.sort(key=lambda r: splitmix64(seed ^ r))
    return sorted(rows[:max_sample_size])


# ---------------------------------------------------------------- one column, all statistics
def collect(tp, values, comparable=False, raw=False, wrap=False, depth=0, width=0, max_fm=1000, max_samples=0, seed=0):
    """values: a list with None for NULL -> dict of everything the collector returns for the column"""
    cells = [bytes(v) if raw else encode_datum(tp, v, comparable) for v in values if v is not None]
    hp = [murmur3_128(e) for e in cells]
    fm_h = [murmur3_64(wrap_bytes(e)) for e in cells] if wrap else [h[0] for h in hp]
    mask, hs = fm_canonical(fm_h, max_fm)
    out = {
        "null_count": sum(v is None for v in values), "count": len(cells), "total_size": sum(len(e) - 1 for e in cells),
        "fm_mask": mask, "fm": sorted(hs), "cm_count": len(cells) if depth else 0,
        "cm": cm_sketch_hashed([h[0] for h in hp], [h[1] for h in hp], depth, width) if depth else None,
    }
    ords = sample_ordinals([v is not None for v in values], seed, max_samples)
    out["sample_ordinals"] = ords
    out["samples"] = [values[r] for r in ords]
    return out


# ---------------------------------------------------------------- SortedBuilder (statistics/builder.go:50-94, histogram.go:155-166, 341-358)
def sorted_builder_rows(values, num_buckets):
    """row by row.  -> (buckets [count, repeat, lower row, upper row], ndv)"""
    b, idx, last, per, ndv = [], 0, 0, 1, 0
    for r, v in enumerate(values):
        if r == 0:
            b.append([1, 1, 0, 0])
            ndv = 1
            continue
        if values[b[idx][3]] == v:
            b[idx][0] += 1
            b[idx][1] += 1
            continue
        if b[idx][0] + 1 - last <= per:
            b[idx] = [b[idx][0] + 1, 1, b[idx][2], r]
        else:
            if idx + 1 == num_buckets:
                m = []
                for i in range(0, idx, 2):
                    m.append([b[i + 1][0], b[i + 1][1], b[i][2], b[i + 1][3]])
                if idx % 2 == 0:
                    m.append(b[idx])
                b = m
                per *= 2
                idx //= 2
                last = 0 if idx == 0 else b[idx - 1][0]
            if b[idx][0] + 1 - last <= per:
                b[idx] = [b[idx][0] + 1, 1, b[idx][2], r]
            else:
                last = b[idx][0]
                idx += 1
                b.append([last + 1, 1, r, r])
        ndv += 1
    return b, ndv


def run_heads(values):
    """before[j] = rows before run j (a run = adjacent equal rows), with the row count appended"""
    before = [r for r in range(len(values)) if r == 0 or values[r] != values[r - 1]]
    return before + [len(values)]


def sorted_builder_runs(values, num_buckets):
    """the run-jump form: a bucket with lastNumber L and width v absorbs run j while before[j] <= L + v - 1"""
    import bisect
    n = len(values)
    if n == 0:
        return [], 0
    before = run_heads(values)
    R = len(before) - 1
    b, idx, L, v, j, fresh = [], 0, 0, 1, 0, True
    while j < R:
        if not fresh:
            if b[idx][0] + 1 - L > v:
                if idx + 1 == num_buckets:
                    m = [[b[i + 1][0], b[i + 1][1], b[i][2], b[i + 1][3]] for i in range(0, idx, 2)]
                    if idx % 2 == 0:
                        m.append(b[idx])
                    b = m
                    v *= 2
                    idx //= 2
                    L = 0 if idx == 0 else b[idx - 1][0]
                if b[idx][0] + 1 - L > v:
                    L = b[idx][0]
                    idx += 1
                    fresh = True
        j2 = bisect.bisect_right(before, L + v - 1, j, R) - 1
        row = [before[j2 + 1], before[j2 + 1] - before[j2], before[j] if fresh else b[idx][2], before[j2]]
        if fresh:
            b.append(row)
        else:
            b[idx] = row
        fresh = False
        j = j2 + 1
    return b, R


# ---------------------------------------------------------------- the deterministic data of the reference's statistics tests
def ref_rc(count=100000, start=1000):
    d = [0] + [2] * (start - 1) + list(range(start, count))
    for i in range(start, count, 3):
        d[i] += 1
    for i in range(start, count, 5):
        d[i] += 2
    return sorted(d)


def ref_samples():
    return ref_rc(10000)


def ref_pk(count=100000):
    return list(range(count))
