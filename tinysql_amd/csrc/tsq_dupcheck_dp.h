// tsq_dupcheck_dp.h — the per-cell and per-key code of the duplicate-key checker (tsq_dupcheck.hip): the order and equality of two
// memcomparable index keys, the lower bound of a key among a store's keys, and EqualDatums of one cell pair.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/dupcheck_dp_main.cpp): a read past a
// key or a cell is found there, not on the GPU.
// Reference: index keys order as bytes.Compare (kv/memdb, store/mockstore/mocktikv): memcmp over the common length, then the shorter
// key first.  EqualDatums is CompareDatum per column (types/datum.go:896-916, types/compare.go:104-123): NULL equals NULL, integers
// by value, doubles with == (-0.0 equals 0.0, a NaN equals nothing), strings by bytes.
#ifndef TSQ_DUPCHECK_DP_H
#define TSQ_DUPCHECK_DP_H

#include "tsq_device.h"

// eight bytes from any byte address, as the big-endian number they spell (so that unsigned order is byte order)
TSQ_HD uint64_t tsq_dc_load_be(const uint8_t* p) {
    uint64_t v;
    __builtin_memcpy(&v, p, 8);
    return __builtin_bswap64(v);
}
// the last n (1..7) bytes of a key, left aligned in a big-endian word; the bytes after them are zero
TSQ_HD uint64_t tsq_dc_load_tail_be(const uint8_t* p, int64_t n) {
    uint64_t v = 0;
    for (int64_t i = 0; i < n; i++) v |= (uint64_t)p[i] << (56 - 8 * i);
    return v;
}
// bytes.Compare: < 0, 0, > 0.  Reads exactly [a, a + la) and [b, b + lb).
TSQ_HD int tsq_dc_key_cmp(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb) {
    const int64_t m = la < lb ? la : lb;
    int64_t i = 0;
    for (; i + 8 <= m; i += 8) {
        const uint64_t x = tsq_dc_load_be(a + i), y = tsq_dc_load_be(b + i);
        if (x != y) return x < y ? -1 : 1;
    }
    if (i < m) {
        const uint64_t x = tsq_dc_load_tail_be(a + i, m - i), y = tsq_dc_load_tail_be(b + i, m - i);
        if (x != y) return x < y ? -1 : 1;
    }
    return la < lb ? -1 : (la > lb ? 1 : 0);
}
// equality alone: the lengths first, then eight bytes at a time
TSQ_HD bool tsq_dc_bytes_equal(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb) {
    if (la != lb) return false;
    int64_t i = 0;
    for (; i + 8 <= la; i += 8)
        if (tsq_dc_load_be(a + i) != tsq_dc_load_be(b + i)) return false;
    if (i < la && tsq_dc_load_tail_be(a + i, la - i) != tsq_dc_load_tail_be(b + i, la - i)) return false;
    return true;
}
// first e in [0, n) whose key (bytes [offs[e], offs[e + 1]) of keys) is >= the probe, n when there is none.  offs must not decrease
// (tsq_dupcheck_create checks it); every index is bounded by n alone.
TSQ_HD int64_t tsq_dc_key_lower(const uint8_t* keys, const int64_t* offs, int64_t n, const uint8_t* probe, int64_t plen) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t b = offs[mid];
        if (tsq_dc_key_cmp(keys + b, offs[mid + 1] - b, probe, plen) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the store entry with exactly the probe's bytes, or -1
TSQ_HD int64_t tsq_dc_key_find(const uint8_t* keys, const int64_t* offs, int64_t n, const uint8_t* probe, int64_t plen) {
    const int64_t e = tsq_dc_key_lower(keys, offs, n, probe, plen);
    if (e >= n) return -1;
    const int64_t b = offs[e];
    return tsq_dc_bytes_equal(keys + b, offs[e + 1] - b, probe, plen) ? e : -1;
}

// one column of one side of tsq_rows_equal
struct tsq_dc_col {
    const void* data;
    const uint8_t* notnull;  // bit = 1: NOT NULL; nullptr: the column holds no NULL
    const int64_t* offsets;  // TSQ_BYTES
    int64_t length;
};
TSQ_HD bool tsq_dc_is_null(const tsq_dc_col& c, int64_t r) { return c.notnull && !((c.notnull[r >> 3] >> (r & 7)) & 1); }
// EqualDatums' verdict on one cell pair of the same column type: row ra of a, row rb of b (both inside their columns)
TSQ_HD bool tsq_dc_cell_equal(int32_t type, const tsq_dc_col& a, int64_t ra, const tsq_dc_col& b, int64_t rb) {
    const bool na = tsq_dc_is_null(a, ra), nb = tsq_dc_is_null(b, rb);
    if (na || nb) return na && nb;
    switch (type) {
        case TSQ_I64:
        case TSQ_U64:
            return ((const uint64_t*)a.data)[ra] == ((const uint64_t*)b.data)[rb];
        case TSQ_F32:
            return ((const float*)a.data)[ra] == ((const float*)b.data)[rb];
        case TSQ_F64:
            return ((const double*)a.data)[ra] == ((const double*)b.data)[rb];
        default: {
            const int64_t oa = a.offsets[ra], ob = b.offsets[rb];
            return tsq_dc_bytes_equal((const uint8_t*)a.data + oa, a.offsets[ra + 1] - oa, (const uint8_t*)b.data + ob, b.offsets[rb + 1] - ob);
        }
    }
}

#endif
