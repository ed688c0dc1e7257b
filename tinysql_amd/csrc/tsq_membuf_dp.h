// tsq_membuf_dp.h — the per-key code of the transaction buffer (tsq_membuf.hip): the checks of one pushed row, the shared prefix, the
// 8-byte images a key is sorted by, the compare, the winner rule among the entries of one key and the search of a Get.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/membuf_dp_main.cpp).
// Reference: kv/memdb_buffer.go (Set :95-108, Delete :111-114), store/tikv/2pc.go initKeysAndMutations (:115-172).
//
// THE ORDER.  bytes.Compare is memcmp over the common length, then the shorter key first.  Behind the prefix all keys share, key k is
// the tuple (image 0, image 1, ..., image D - 1, tail): image d = bytes [8 d, 8 d + 8) behind the prefix as a big-endian number,
// ZERO-PADDED where the key ends inside or before the window; tail = (length << 1) | (1 when the entry is not a lock).  The tuples
// order as bytes.Compare does: where the padded images first differ inside both keys memcmp decides; where they first differ behind
// the end of the shorter key, that key holds a zero where the longer holds a non-zero byte and is a proper prefix of it; where no image
// differs the keys differ in trailing 0x00 bytes alone ("ab", "ab\0", "ab\0\0") and the length decides — which is why the length is
// part of the tie-break and not left to the sequence number.  Entries with equal keys then come lock entries first, each group in
// sequence order (the sort is stable and starts from it): THE LAST ENTRY OF A RUN OF EQUAL KEYS IS THE WINNER — the latest Set or
// Delete if there is one, else the latest lock.
// Every index below is bounded by the counts of the buffer, never by the data.
#ifndef TSQ_MEMBUF_DP_H
#define TSQ_MEMBUF_DP_H

#include "tsq_dupcheck_dp.h"  // tsq_dc_key_cmp, tsq_dc_load_be, tsq_dc_load_tail_be

// bits of the push checks (mb_push_message of tsq_membuf.hip picks the message in its own order)
#define TSQ_MB_E_OFFSETS 1u     // an offset pair that decreases or leaves its buffer
#define TSQ_MB_E_EMPTY_KEY 2u
#define TSQ_MB_E_NIL_VALUE 4u   // ErrCannotSetNilValue
#define TSQ_MB_E_TOO_LARGE 8u   // ErrEntryTooLarge

// one push as its rows see it
struct tsq_mb_push_view {
    const int64_t* koff;  // [n + 1], or NULL: keys of fixed_len bytes
    int64_t fixed_len;
    int64_t key_bytes;
    const int64_t* voff;  // SET: [n + 1]
    int64_t value_bytes;
    int64_t n;
    int32_t kind;         // TSQ_MEMBUF_*
    int64_t entry_limit;  // 0: none
};

TSQ_HD bool tsq_mb_pair_ok(const int64_t* offs, int64_t i, int64_t n_bytes) {
    const int64_t b = offs[i], t = offs[i + 1];
    return b >= 0 && b <= t && t <= n_bytes;
}

// row i of a push: its error bits; where its key and value lie in the push's bytes (valid when the bits are zero)
TSQ_HD uint32_t tsq_mb_push_check(const tsq_mb_push_view& p, int64_t i, int64_t* kbeg, int64_t* klen, int64_t* vbeg, int64_t* vlen) {
    *kbeg = *klen = *vbeg = *vlen = 0;
    if (p.koff) {
        if (!tsq_mb_pair_ok(p.koff, i, p.key_bytes)) return TSQ_MB_E_OFFSETS;
        *kbeg = p.koff[i];
        *klen = p.koff[i + 1] - p.koff[i];
    } else {
        if (p.fixed_len < 0 || (i + 1) * p.fixed_len > p.key_bytes) return TSQ_MB_E_OFFSETS;
        *kbeg = i * p.fixed_len;
        *klen = p.fixed_len;
    }
    if (p.kind == TSQ_MEMBUF_SET) {
        if (!tsq_mb_pair_ok(p.voff, i, p.value_bytes)) return TSQ_MB_E_OFFSETS;
        *vbeg = p.voff[i];
        *vlen = p.voff[i + 1] - p.voff[i];
    }
    uint32_t e = 0;
    if (*klen == 0) e |= TSQ_MB_E_EMPTY_KEY;
    if (p.kind == TSQ_MEMBUF_SET) {
        if (*vlen == 0) e |= TSQ_MB_E_NIL_VALUE;
        else if (p.entry_limit > 0 && *klen + *vlen > p.entry_limit) e |= TSQ_MB_E_TOO_LARGE;
    }
    return e;
}

// the number of leading bytes two keys share, at most `cap`
TSQ_HD int64_t tsq_mb_common_prefix(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb, int64_t cap) {
    int64_t m = la < lb ? la : lb;
    m = m < cap ? m : cap;
    int64_t i = 0;
    for (; i + 8 <= m; i += 8) {
        const uint64_t x = tsq_dc_load_be(a + i) ^ tsq_dc_load_be(b + i);
        if (x) return i + (__builtin_clzll(x) >> 3);
    }
    for (; i < m; i++)
        if (a[i] != b[i]) return i;
    return m;
}

// image `depth` of a key behind `prefix` shared bytes (prefix <= len): zero-padded behind the key's end
TSQ_HD uint64_t tsq_mb_image(const uint8_t* key, int64_t len, int64_t prefix, int64_t depth) {
    const int64_t at = prefix + 8 * depth, left = len - at;
    if (left <= 0) return 0;
    return left >= 8 ? tsq_dc_load_be(key + at) : tsq_dc_load_tail_be(key + at, left);
}
// the tail of the tuple: the length behind the prefix, then lock entries in front of the Sets and Deletes of the same key
TSQ_HD uint64_t tsq_mb_tail_image(int64_t len, int64_t prefix, int32_t kind) {
    return ((uint64_t)(len - prefix) << 1) | (kind == TSQ_MEMBUF_LOCK ? 0u : 1u);
}
// the number of images of the longest key
TSQ_HD int64_t tsq_mb_depths(int64_t max_len, int64_t prefix) { return max_len > prefix ? (max_len - prefix + 7) / 8 : 0; }

// the order of two entries as the sort leaves them: the tuple, then the sequence number.  (The radix passes do not call it: they
// sort by the tuple's digits.  The host test holds the passes' order to it and it to bytes.Compare.)
TSQ_HD int tsq_mb_entry_cmp(const uint8_t* a, int64_t la, int32_t ka, int64_t sa, const uint8_t* b, int64_t lb, int32_t kb, int64_t sb, int64_t prefix,
                            int64_t depths) {
    for (int64_t d = 0; d < depths; d++) {
        const uint64_t x = tsq_mb_image(a, la, prefix, d), y = tsq_mb_image(b, lb, prefix, d);
        if (x != y) return x < y ? -1 : 1;
    }
    const uint64_t x = tsq_mb_tail_image(la, prefix, ka), y = tsq_mb_tail_image(lb, prefix, kb);
    if (x != y) return x < y ? -1 : 1;
    return sa < sb ? -1 : (sa > sb ? 1 : 0);
}

// bytes.Equal of two keys that share `prefix` bytes
TSQ_HD bool tsq_mb_key_equal(const uint8_t* a, int64_t la, const uint8_t* b, int64_t lb, int64_t prefix) {
    if (la != lb) return false;
    return tsq_dc_key_cmp(a + prefix, la - prefix, b + prefix, lb - prefix) == 0;
}

// the sorted entries as the winner rule sees them
struct tsq_mb_sorted {
    const uint8_t* keys;
    const int64_t* kbeg;   // by entry
    const int64_t* klen;
    const uint32_t* order; // [n]: the entry at every sorted position
    int64_t n;
    int64_t prefix;
};
// the entry at sorted position i survives: it is the last of its run of equal keys
TSQ_HD bool tsq_mb_is_winner(const tsq_mb_sorted& s, int64_t i) {
    if (i + 1 >= s.n) return true;
    const uint32_t e = s.order[i], f = s.order[i + 1];
    return !tsq_mb_key_equal(s.keys + s.kbeg[e], s.klen[e], s.keys + s.kbeg[f], s.klen[f], s.prefix);
}
// entries e - 1 and e arrived strictly ascending (e >= 1)
TSQ_HD bool tsq_mb_ascending_at(const uint8_t* keys, const int64_t* kbeg, const int64_t* klen, int64_t e) {
    return tsq_dc_key_cmp(keys + kbeg[e - 1], klen[e - 1], keys + kbeg[e], klen[e]) < 0;
}

// memDbBuffer.Get over the finished entries (strictly ascending): the index of the key or -1
TSQ_HD int64_t tsq_mb_find(const uint8_t* keys, const int64_t* koff, int64_t m, const uint8_t* probe, int64_t plen) {
    int64_t lo = 0, hi = m;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tsq_dc_key_cmp(keys + koff[mid], koff[mid + 1] - koff[mid], probe, plen) < 0) lo = mid + 1;
        else hi = mid;
    }
    if (lo < m && tsq_dc_key_cmp(keys + koff[lo], koff[lo + 1] - koff[lo], probe, plen) == 0) return lo;
    return -1;
}

#endif
