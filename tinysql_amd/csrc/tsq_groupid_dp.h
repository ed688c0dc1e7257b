// tsq_groupid_dp.h — the GROUP KEY CELL of tsq_groupid (tsq_groupid.hip): host/device-portable (TSQ_HD), so that the CPU suite compiles
// the same code into a stand-alone program.  Two rows belong to one group iff their key cells are equal column by column, as
// getGroupKey / codec.HashGroupKey define it (executor/aggregate.go:359-394, util/codec/codec.go:713-746):
//   NULL    : a value of its own (NilFlag) — not 0, not ""
//   I64/U64 : the 8 bytes (the UNSIGNED flag is ignored: codec.go:715-723)
//   F32     : widened to double, then as F64
//   F64     : the memcomparable image (util/codec/float.go:22-30): -0.0 and +0.0 share a group, NaNs group by their bits
//   BYTES   : length and bytes (compactBytesFlag + varint(len) + bytes, codec.go:738-744)
// A row's hash only chooses where the walk through the table starts and which slots are worth a comparison: equality is decided on
// the cells (gid_rows_equal), never on the hash.  No array is indexed by a run-time value here: the column loop carries the hash /
// the verdict alone.
#ifndef TSQ_GROUPID_DP_H
#define TSQ_GROUPID_DP_H

#include "tsq_device.h"

// the word image of a non-NULL fixed-width cell (what group_key_word of tsq_agg.hip states for the four-key routes)
TSQ_HD uint64_t gid_real_image(double f) {
    const uint64_t u = tsq_f64_bits(f);
    return f >= 0 ? (u | 0x8000000000000000ULL) : ~u;  // float.go:22-30 (-0.0 >= 0 is true)
}
TSQ_HD uint64_t gid_word_image(int32_t type, const void* data, int64_t row) {
    if (type == TSQ_F32) return gid_real_image((double)((const float*)data)[row]);
    if (type == TSQ_F64) return gid_real_image(((const double*)data)[row]);
    return ((const uint64_t*)data)[row];
}

TSQ_HD bool gid_bytes_equal(const uint8_t* a, const uint8_t* b, int64_t n) {
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t x, y;
        memcpy(&x, a + i, 8);
        memcpy(&y, b + i, 8);
        if (x != y) return false;
    }
    for (; i < n; i++)
        if (a[i] != b[i]) return false;
    return true;
}

// cell (c, ra) of `a` against cell (c, rb) of `b`; both sets have the same column types
TSQ_HD bool gid_cell_equal(const tsq_colset& a, int64_t ra, const tsq_colset& b, int64_t rb, int c) {
    const bool na = tsq_is_null(a.nulls[c], ra), nb = tsq_is_null(b.nulls[c], rb);
    if (na || nb) return na && nb;
    const int32_t t = a.type[c];
    if (t == TSQ_BYTES) {
        const int64_t oa = a.offs[c][ra], ob = b.offs[c][rb];
        const int64_t la = a.offs[c][ra + 1] - oa, lb = b.offs[c][rb + 1] - ob;
        return la == lb && gid_bytes_equal((const uint8_t*)a.data[c] + oa, (const uint8_t*)b.data[c] + ob, la);
    }
    return gid_word_image(t, a.data[c], ra) == gid_word_image(t, b.data[c], rb);
}
TSQ_HD bool gid_rows_equal(const tsq_colset& a, int64_t ra, const tsq_colset& b, int64_t rb) {
    for (int c = 0; c < a.n; c++)
        if (!gid_cell_equal(a, ra, b, rb, c)) return false;
    return true;
}

// equal cells hash alike (the image is hashed, not the stored bits); the column number enters, so that column permutations of a
// key start their walks at different slots
TSQ_HD uint64_t gid_cell_hash(const tsq_colset& a, int64_t row, int c) {
    if (tsq_is_null(a.nulls[c], row)) return TSQ_ROWHASH_NULL;
    if (a.type[c] == TSQ_BYTES) {
        const int64_t o = a.offs[c][row];
        return tsq_hash_bytes((const uint8_t*)a.data[c] + o, a.offs[c][row + 1] - o);
    }
    return gid_word_image(a.type[c], a.data[c], row);
}
TSQ_HD uint64_t gid_row_hash(const tsq_colset& a, int64_t row) {
    uint64_t h = TSQ_ROWHASH_SEED;
    for (int c = 0; c < a.n; c++) h = tsq_rowhash_step(h, gid_cell_hash(a, row, c), (uint32_t)c);
    return h;
}

// a table slot: [63:32] tag — the high half of the (possibly truncated) row hash with bit 31 set, so that an occupied slot is never
// 0 — and [31:0] the group id, or while the slice that brought the key is in flight, base + the smallest slice row seen with this key
TSQ_HD uint64_t gid_slot_tag(uint64_t h) { return ((h >> 32) | 0x80000000ULL) << 32; }

#endif
