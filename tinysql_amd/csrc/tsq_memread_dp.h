// tsq_memread_dp.h — the per-position code of the mem readers' scan of the finished transaction buffer (tsq_memread.hip): the bound
// of one range end among the buffer's keys, the verdict of one point key, position -> (range, entry), the keep rule, where a kept
// pair goes for an ascending and a descending scan, and the handle of one record key of the dirty-handle pass.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/memread_dp_main.cpp).
// Reference: executor/mem_reader.go iterTxnMemBuffer (:256-281) over memDbBuffer.Iter (kv/memdb_buffer.go:51-65, Valid :142-147);
// reverseDatumSlice over the rows of ALL ranges (:129-131, :206-208); executor/union_scan.go DirtyTable (:56-74).
//
// A POSITION is one entry one range examines: range r owns the positions [rbase[r], rbase[r + 1]) and position p of it is entry
// rlo[r] + (p - rbase[r]) of the buffer.  Overlapping ranges examine an entry once each.  A point key is a range of one or no entry.
// Every index below is bounded by the counts of the buffer and of the call, never by the data.
#ifndef TSQ_MEMREAD_DP_H
#define TSQ_MEMREAD_DP_H

#include "tsq_membuf_dp.h"  // tsq_mb_pair_ok; tsq_dc_key_cmp, tsq_dc_bytes_equal, tsq_dc_key_lower, tsq_dc_load_be

#define TSQ_MR_E_OFFSETS 1u      // an offset pair that decreases or leaves its buffer
#define TSQ_MR_E_INVALID_KEY 2u  // a key of a table's record range that is not RecordRowKeyLen long
#define TSQ_MR_ROWKEY_LEN 19

// the finished buffer as a reader sees it: m strictly ascending keys, their ops, the value offsets
struct tsq_mr_buffer {
    const uint8_t* okeys;
    const int64_t* okoff;  // [m + 1]
    const uint8_t* oops;   // TSQ_MVCC_OP_PUT / DEL / LOCK
    const int64_t* ovoff;  // [m + 1]
    int64_t m;
};

// Bound j (0 <= j < 2 n_ranges) of a range list laid out as tsq_mvcc_scan's: j = 2 r is range r's start, j = 2 r + 1 its end.  The
// index of the first entry at or above the bound; an empty start is the first key, an empty end "to the last key" (the pinned
// departure of include/tsq.h).  A bad offset pair sets the error bit and answers 0.
TSQ_HD int64_t tsq_mr_range_bound(const tsq_mr_buffer& b, const uint8_t* rbytes, const int64_t* roffs, int64_t j, uint32_t* err) {
    const int64_t lo = roffs[j], hi = roffs[j + 1];
    if (lo < 0 || hi < lo) {
        *err |= TSQ_MR_E_OFFSETS;
        return 0;
    }
    if (hi == lo) return (j & 1) ? b.m : 0;
    return tsq_dc_key_lower(b.okeys, b.okoff, b.m, rbytes + lo, hi - lo);
}
// the entries between the two bounds of one range: start >= end selects nothing
TSQ_HD int64_t tsq_mr_range_count(int64_t lo, int64_t hi) { return hi > lo ? hi - lo : 0; }

// Point key i, passed as in a push (koff NULL: keys of fixed_len bytes): the entry at or above it, and 1 when that entry IS the key
TSQ_HD int64_t tsq_mr_point(const tsq_mr_buffer& b, const uint8_t* keys, const int64_t* koff, int64_t fixed_len, int64_t key_bytes, int64_t i, int64_t* count,
                            uint32_t* err) {
    *count = 0;
    int64_t kb, kl;
    if (koff) {
        if (!tsq_mb_pair_ok(koff, i, key_bytes)) {
            *err |= TSQ_MR_E_OFFSETS;
            return 0;
        }
        kb = koff[i], kl = koff[i + 1] - kb;
    } else {
        if (fixed_len < 0 || (i + 1) * fixed_len > key_bytes) {
            *err |= TSQ_MR_E_OFFSETS;
            return 0;
        }
        kb = i * fixed_len, kl = fixed_len;
    }
    const int64_t e = tsq_dc_key_lower(b.okeys, b.okoff, b.m, keys + kb, kl);
    if (e < b.m && tsq_dc_bytes_equal(b.okeys + b.okoff[e], b.okoff[e + 1] - b.okoff[e], keys + kb, kl)) *count = 1;
    return e;
}

// the range that owns position p: the last r in [0, n_ranges) with rbase[r] <= p (rbase: n_ranges + 1 entries, not decreasing, n_ranges >= 1)
TSQ_HD int64_t tsq_mr_range_of(const int64_t* rbase, int64_t n_ranges, int64_t p) {
    int64_t lo = 0, hi = n_ranges;  // the first r with rbase[r] > p lies in (lo .. hi]
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (rbase[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo > 0 ? lo - 1 : 0;
}

// Position p: its entry (-1 when the range arrays contradict the buffer's count: nothing is read), whether it yields a pair — only a
// PUT does: a DEL is the reference's len(iter.Value()) == 0, a lock-only key is not in the reference's buffer at all — whether it is a
// skipped delete, and the pair's key and value lengths (0 when it yields none).
TSQ_HD bool tsq_mr_mark(const tsq_mr_buffer& b, const int64_t* rlo, const int64_t* rbase, int64_t n_ranges, int64_t p, int64_t* entry, bool* del, int64_t* klen,
                        int64_t* vlen) {
    *entry = -1, *del = false, *klen = *vlen = 0;
    const int64_t r = tsq_mr_range_of(rbase, n_ranges, p);
    const int64_t e = rlo[r] + (p - rbase[r]);
    if (p < rbase[r] || e < 0 || e >= b.m) return false;
    *entry = e;
    const uint8_t op = b.oops[e];
    *del = op == TSQ_MVCC_OP_DEL;
    if (op != TSQ_MVCC_OP_PUT) return false;
    *klen = b.okoff[e + 1] - b.okoff[e];
    *vlen = b.ovoff[e + 1] - b.ovoff[e];
    return true;
}

// Where the pair with ordinal `ord` (among n_pairs, in ascending scan order) goes: its place in the result and the first byte of a
// cell that begins at byte `beg` of the ascending layout and is `len` long, out of `total` bytes.  desc reverses the WHOLE sequence,
// so the offsets are the suffix form of the ascending ones: no second scan.
TSQ_HD int64_t tsq_mr_place(int64_t ord, int64_t n_pairs, int32_t desc) { return desc ? n_pairs - 1 - ord : ord; }
TSQ_HD int64_t tsq_mr_place_bytes(int64_t beg, int64_t len, int64_t total, int32_t desc) { return desc ? total - beg - len : beg; }

// the record range of a table: 't' | EncodeInt(table_id) | "_r" (end = 0) or "_s" (end = 1), 11 bytes
TSQ_HD void tsq_mr_record_bound(int64_t table_id, int end, uint8_t* out11) {
    const uint64_t t = (uint64_t)table_id ^ 0x8000000000000000ULL;
    out11[0] = (uint8_t)'t';
    for (int i = 0; i < 8; i++) out11[1 + i] = (uint8_t)(t >> (56 - 8 * i));
    out11[9] = (uint8_t)'_';
    out11[10] = (uint8_t)(end ? 's' : 'r');
}
// Entry e of the record range: its op and its handle (DecodeRowKey: the last 8 of 19 bytes, big-endian, sign bit flipped); a key of
// another length sets the error bit
TSQ_HD uint8_t tsq_mr_dirty_at(const tsq_mr_buffer& b, int64_t e, int64_t* handle, uint32_t* err) {
    *handle = 0;
    const int64_t kb = b.okoff[e], kl = b.okoff[e + 1] - kb;
    if (kl != TSQ_MR_ROWKEY_LEN) {
        *err |= TSQ_MR_E_INVALID_KEY;
        return TSQ_MVCC_OP_LOCK;  // (goes to neither list)
    }
    *handle = (int64_t)(tsq_dc_load_be(b.okeys + kb + 11) ^ 0x8000000000000000ULL);
    return b.oops[e];
}

#endif
