// tsq_rowenc_dp.h — the scalar core of the write path (tsq_rowenc.hip): one cell -> its stored-row value bytes, the header fields and
// length of a stored row (row format v2), and the rune walk of an index prefix.  TSQ_HD so that the CPU test-suite compiles the very
// same code on the host (tests/rowenc_dp_main.cpp) against the CPU restatement that is pinned on the reference's vectors.
// Reference: Encoder.Encode / reformatCols / encodeRowCols / EncodeValueDatum (util/rowcodec/encoder.go:34-194), encodeInt / encodeUint
// (util/rowcodec/common.go:84-101, 180-197), codec.EncodeFloat (util/codec/float.go:22-30), row.toBytes (util/rowcodec/row.go:80-99),
// TruncateIndexValuesIfNeeded (table/tables/index.go:127-157) with Go's utf8.DecodeRune / bytes.Runes.
#ifndef TSQ_ROWENC_DP_H
#define TSQ_ROWENC_DP_H

#include "tsq_device.h"

// bytes encodeInt / encodeUint write: the narrowest of 1, 2, 4, 8 that holds the value
TSQ_HD uint32_t tsq_re_int_width(int64_t v) {
    if ((int64_t)(int8_t)v == v) return 1u;
    if ((int64_t)(int16_t)v == v) return 2u;
    if ((int64_t)(int32_t)v == v) return 4u;
    return 8u;
}
TSQ_HD uint32_t tsq_re_uint_width(uint64_t v) {
    if (v <= 0xffu) return 1u;
    if (v <= 0xffffu) return 2u;
    if (v <= 0xffffffffu) return 4u;
    return 8u;
}

// the value bytes of a NOT NULL fixed-width cell: byte k of the value = (*le >> 8k); returns their count.
// bits: the column's 8 bytes (a float column: the DOUBLE image of the value, the caller widens float32 first)
TSQ_HD uint32_t tsq_re_value(int32_t type, uint64_t bits, uint64_t* le) {
    if (type == TSQ_F32 || type == TSQ_F64) {
        // encodeFloatToCmpUint64 decides on the VALUE: -0.0 is ">= 0", a NaN is not; EncodeUint writes big endian
        const uint64_t u = (tsq_bits_f64(bits) >= 0) ? (bits | 0x8000000000000000ULL) : ~bits;
        *le = ((uint64_t)__builtin_bswap32((uint32_t)(u >> 32))) | ((uint64_t)__builtin_bswap32((uint32_t)u) << 32);
        return 8u;
    }
    *le = bits;  // little endian, cut to the width
    return type == TSQ_I64 ? tsq_re_int_width((int64_t)bits) : tsq_re_uint_width(bits);
}

// a bit column's cell (TSQ_RC_BIT): 1..8 big-endian bytes -> the unsigned integer they spell (stored like a TSQ_U64 value, what
// tsq_rowcodec_decode turns back into the cell).  false: any other cell length
TSQ_HD bool tsq_re_bit_value(const uint8_t* p, uint64_t n, uint64_t* v) {
    *v = 0;
    if (n < 1 || n > 8) return false;
    uint64_t u = 0;
    for (uint64_t i = 0; i < n; i++) u = (u << 8) | p[i];
    *v = u;
    return true;
}

// A row is large (u32 ids and offsets) when a column id exceeds 255 or its value bytes pass 65535.  DEPARTURE from the reference
// at EXACTLY 65535 value bytes: there it turns the row large without widening its offsets (encoder.go:151-157) and the row cannot
// be decoded; here such a row is large with the offsets it means.
TSQ_HD bool tsq_re_large(bool any_id_large, uint64_t value_bytes) { return any_id_large || value_bytes >= 65535u; }

// row.toBytes: [128][large][numNotNull u16][numNull u16] | ids | end offsets of the not-null values | values
TSQ_HD uint64_t tsq_re_row_len(bool large, uint32_t n_notnull, uint32_t n_null, uint64_t value_bytes) {
    return 6u + (uint64_t)(n_notnull + n_null) * (large ? 4u : 1u) + (uint64_t)n_notnull * (large ? 4u : 2u) + value_bytes;
}
// the six header bytes, byte k = (result >> 8k)
TSQ_HD uint64_t tsq_re_header(bool large, uint32_t n_notnull, uint32_t n_null) {
    return 128u | ((uint64_t)(large ? 1u : 0u) << 8) | ((uint64_t)(n_notnull & 0xffffu) << 16) | ((uint64_t)(n_null & 0xffffu) << 32);
}

// utf8.DecodeRune at p[0 .. n), n >= 1: the width of the rune there.  A byte that does not start a shortest-form, non-surrogate
// sequence up to U+10FFFF (or whose sequence is cut short) is one rune of width 1 with *valid = false (Go's RuneError, 1)
TSQ_HD uint32_t tsq_re_rune_width(const uint8_t* p, uint64_t n, bool* valid) {
    const uint8_t b0 = p[0];
    *valid = true;
    if (b0 < 0x80u) return 1u;
    uint32_t need;       // continuation bytes
    uint8_t lo = 0x80u, hi = 0xBFu;  // the range of the FIRST continuation byte
    if (b0 >= 0xC2u && b0 <= 0xDFu) need = 1;
    else if (b0 >= 0xE0u && b0 <= 0xEFu) {
        need = 2;
        if (b0 == 0xE0u) lo = 0xA0u;       // no overlong forms
        else if (b0 == 0xEDu) hi = 0x9Fu;  // no surrogates
    } else if (b0 >= 0xF0u && b0 <= 0xF4u) {
        need = 3;
        if (b0 == 0xF0u) lo = 0x90u;
        else if (b0 == 0xF4u) hi = 0x8Fu;  // up to U+10FFFF
    } else {
        *valid = false;
        return 1u;
    }
    if (n < (uint64_t)need + 1u || p[1] < lo || p[1] > hi) { *valid = false; return 1u; }
    for (uint32_t i = 2; i <= need; i++) {
        if (p[i] < 0x80u || p[i] > 0xBFu) { *valid = false; return 1u; }
    }
    return need + 1u;
}

// the first `k` runes of the cell p[0 .. n): the bytes they span.  *truncated: the cell holds more than k runes (only then the
// reference touches it); *bad: one of the kept runes is an invalid byte (the reference would rewrite it as EF BF BD)
TSQ_HD uint64_t tsq_re_rune_prefix(const uint8_t* p, uint64_t n, uint64_t k, bool* truncated, bool* bad) {
    uint64_t pos = 0;
    bool any_bad = false;
    for (uint64_t i = 0; i < k && pos < n; i++) {
        bool ok;
        pos += tsq_re_rune_width(p + pos, n - pos, &ok);
        any_bad = any_bad || !ok;
    }
    *truncated = pos < n;
    *bad = any_bad && pos < n;
    return pos;
}

// TruncateIndexValuesIfNeeded for one var-len cell: the bytes of it the index key holds.  prefix_len < 0: the whole cell
TSQ_HD uint64_t tsq_re_index_cell_len(const uint8_t* p, uint64_t n, int64_t prefix_len, bool utf8, bool* bad) {
    *bad = false;
    if (prefix_len < 0) return n;
    if (!utf8) return n > (uint64_t)prefix_len ? (uint64_t)prefix_len : n;
    if (n <= (uint64_t)prefix_len) return n;  // at most n runes: nothing to cut, no need to walk
    bool truncated;
    return tsq_re_rune_prefix(p, n, (uint64_t)prefix_len, &truncated, bad);
}

// number of runes of a cell (utf8.RuneCount) — the test's view of the walk
TSQ_HD uint64_t tsq_re_rune_count(const uint8_t* p, uint64_t n) {
    uint64_t pos = 0, cnt = 0;
    while (pos < n) {
        bool ok;
        pos += tsq_re_rune_width(p + pos, n - pos, &ok);
        cnt++;
    }
    return cnt;
}

#endif
