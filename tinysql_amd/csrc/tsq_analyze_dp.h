// tsq_analyze_dp.h — the scalar core of the ANALYZE collector (tsq_analyze.hip): the byte string of a cell, its murmur3 hashes and the
// sampling key.  TSQ_HD like tsq_encode_dp.h, whose datum forms it reuses.
// Reference: SampleCollector.collect (statistics/sample.go:143-177), FMSketch.InsertValue (statistics/fmsketch.go:65-77: murmur3.New64 of
// the datum's encoded bytes), CMSketch.QueryBytes (statistics/cmsketch.go:63-67: murmur3.Sum128), codec.encode (util/codec/codec.go:74-109).
// murmur3 is the public x64_128 variant (Austin Appleby's MurmurHash3, seed 0); Sum64 of the 64-bit hasher is its first word.
#ifndef TSQ_ANALYZE_DP_H
#define TSQ_ANALYZE_DP_H

#include "tsq_encode_dp.h"

#define TSQ_MM3_C1 0x87c37b91114253d5ULL
#define TSQ_MM3_C2 0x4cf5ad432745937fULL

TSQ_HD uint64_t tsq_rotl64(uint64_t x, int r) { return (x << r) | (x >> (64 - r)); }
TSQ_HD uint64_t tsq_mm3_fmix(uint64_t k) {
    k ^= k >> 33;
    k *= 0xff51afd7ed558ccdULL;
    k ^= k >> 33;
    k *= 0xc4ceb9fe1a85ec53ULL;
    k ^= k >> 33;
    return k;
}
struct tsq_mm3 {
    uint64_t h1, h2;
};
// one 16-byte block: k1 = bytes 0..7, k2 = bytes 8..15, little endian
TSQ_HD void tsq_mm3_block(tsq_mm3& s, uint64_t k1, uint64_t k2) {
    k1 *= TSQ_MM3_C1;
    k1 = tsq_rotl64(k1, 31);
    k1 *= TSQ_MM3_C2;
    s.h1 ^= k1;
    s.h1 = tsq_rotl64(s.h1, 27);
    s.h1 += s.h2;
    s.h1 = s.h1 * 5 + 0x52dce729ULL;
    k2 *= TSQ_MM3_C2;
    k2 = tsq_rotl64(k2, 33);
    k2 *= TSQ_MM3_C1;
    s.h2 ^= k2;
    s.h2 = tsq_rotl64(s.h2, 31);
    s.h2 += s.h1;
    s.h2 = s.h2 * 5 + 0x38495ab5ULL;
}
// the last len & 15 bytes, zero padded in (k1, k2) — a zero word mixes to zero, so the tail needs no length test — and the finalizer
TSQ_HD void tsq_mm3_finish(tsq_mm3& s, uint64_t k1, uint64_t k2, uint64_t len) {
    k2 *= TSQ_MM3_C2;
    k2 = tsq_rotl64(k2, 33);
    k2 *= TSQ_MM3_C1;
    s.h2 ^= k2;
    k1 *= TSQ_MM3_C1;
    k1 = tsq_rotl64(k1, 31);
    k1 *= TSQ_MM3_C2;
    s.h1 ^= k1;
    s.h1 ^= len;
    s.h2 ^= len;
    s.h1 += s.h2;
    s.h2 += s.h1;
    s.h1 = tsq_mm3_fmix(s.h1);
    s.h2 = tsq_mm3_fmix(s.h2);
    s.h1 += s.h2;
    s.h2 += s.h1;
}
// a string of at most 15 bytes held in two words: a fixed-width datum (<= 11 bytes), also wrapped (<= 13)
TSQ_HD tsq_mm3 tsq_mm3_short(uint64_t lo, uint64_t hi, uint32_t len) {
    tsq_mm3 s = {0, 0};
    tsq_mm3_finish(s, lo, hi, len);
    return s;
}

// A byte string made of up to 24 prefix bytes (little endian in p0..p2) and a body: the bytes of a var-len cell, or (mem) the
// memcomparable groups of that cell (tsq_enc_membytes_at).  Nothing is materialised: the hash reads byte by byte.
struct tsq_an_bytes {
    uint64_t p0, p1, p2;
    uint32_t npre;
    uint32_t mem;
    const uint8_t* src;
    uint64_t n;      // bytes of the cell
    uint64_t nbody;  // bytes of the body
};
TSQ_HD void tsq_an_pre_put(tsq_an_bytes& b, uint64_t lo, uint32_t hi, uint32_t len) {
    for (uint32_t i = 0; i < len; i++) {
        const uint64_t byte = i < 8 ? (lo >> (8 * i)) & 0xff : ((uint64_t)hi >> (8 * (i - 8))) & 0xff;
        const uint32_t at = b.npre + i, sh = 8 * (at & 7);
        if (at < 8) b.p0 |= byte << sh;
        else if (at < 16) b.p1 |= byte << sh;
        else b.p2 |= byte << sh;
    }
    b.npre += len;
}
TSQ_HD uint64_t tsq_an_len(const tsq_an_bytes& b) { return b.npre + b.nbody; }
TSQ_HD uint64_t tsq_an_at(const tsq_an_bytes& b, uint64_t i) {
    if (i < b.npre) {
        const uint64_t w = i < 8 ? b.p0 : (i < 16 ? b.p1 : b.p2);
        return (w >> (8 * (i & 7))) & 0xff;
    }
    i -= b.npre;
    return b.mem ? tsq_enc_membytes_at(b.src, b.n, i) : b.src[i];
}
// e of a var-len cell: raw -> the cell itself; comparable -> bytesFlag + memcomparable groups; else compactBytesFlag + varint(n) + bytes
TSQ_HD tsq_an_bytes tsq_an_cell(const uint8_t* src, uint64_t n, bool raw, bool comparable) {
    tsq_an_bytes b = {0, 0, 0, 0, 0, src, n, n};
    if (raw) return b;
    if (comparable) {
        b.p0 = 1;  // bytesFlag
        b.npre = 1;
        b.mem = 1;
        b.nbody = tsq_enc_membytes_len(n) - 1;
        return b;
    }
    uint64_t lo;
    uint32_t hi;
    const uint32_t hl = tsq_enc_str_hdr(n, &lo, &hi);
    tsq_an_pre_put(b, lo, hi, hl);
    return b;
}
// the bytes datum of e as the storage side sees it (TSQ_AN_WRAP_BYTES): compactBytesFlag + varint(len e) + e
TSQ_HD tsq_an_bytes tsq_an_wrap(const tsq_an_bytes& e) {
    tsq_an_bytes w = {0, 0, 0, 0, e.mem, e.src, e.n, e.nbody};
    uint64_t lo;
    uint32_t hi;
    const uint32_t hl = tsq_enc_str_hdr(tsq_an_len(e), &lo, &hi);
    tsq_an_pre_put(w, lo, hi, hl);
    tsq_an_pre_put(w, e.p0, (uint32_t)e.p1, e.npre);  // (e.npre <= 11)
    return w;
}
TSQ_HD tsq_mm3 tsq_an_hash(const tsq_an_bytes& b) {
    tsq_mm3 s = {0, 0};
    const uint64_t len = tsq_an_len(b);
    uint64_t i = 0;
    for (; i + 16 <= len; i += 16) {
        uint64_t k1 = 0, k2 = 0;
        for (uint32_t j = 0; j < 8; j++) {
            k1 |= tsq_an_at(b, i + j) << (8 * j);
            k2 |= tsq_an_at(b, i + 8 + j) << (8 * j);
        }
        tsq_mm3_block(s, k1, k2);
    }
    uint64_t k1 = 0, k2 = 0;
    for (uint32_t j = 0; i + j < len; j++) {
        if (j < 8) k1 |= tsq_an_at(b, i + j) << (8 * j);
        else k2 |= tsq_an_at(b, i + j) << (8 * (j - 8));
    }
    tsq_mm3_finish(s, k1, k2, len);
    return s;
}

// a fixed-width datum e = (lo, hi, len <= 11) wrapped: [2][varint(len) = 2 * len, one byte] + e
TSQ_HD tsq_mm3 tsq_an_hash_fixed_wrapped(uint64_t lo, uint32_t hi, uint32_t len) {
    const uint64_t k1 = 2ull | ((uint64_t)(2u * len) << 8) | (lo << 16);
    const uint64_t k2 = (lo >> 48) | ((uint64_t)hi << 16);
    return tsq_mm3_short(k1, k2, len + 2u);
}

// counter i of sketch row i (upstream TiDB's CMSketch.insertBytesByCount): uint64 wrap-around, then mod width
TSQ_HD uint32_t tsq_an_cm_index(uint64_t h1, uint64_t h2, uint32_t i, uint32_t width) { return (uint32_t)((h1 + h2 * (uint64_t)i) % (uint64_t)width); }

// the sampling key of row ordinal r: the sample of a column = its non-NULL rows with the smallest keys
TSQ_HD uint64_t tsq_an_sample_key(uint64_t seed, uint64_t r) { return tsq_splitmix64(seed ^ r); }

TSQ_HD int tsq_an_tz(uint64_t h) { return h ? __builtin_ctzll(h) : 64; }

#endif
