// tsq_device.h — scalar building blocks shared by every HIP kernel of libtsq.
//
// Everything here is TSQ_HD (__host__ __device__) and free of HIP runtime calls so that the
// exact same source can be compiled by g++ into tests/hostsim (a test-only shared object that
// checks the per-row semantics against the oracle without a GPU).  The product never uses a
// host build of these functions: libtsq's entry points launch HIP kernels or fail loudly.
#ifndef TSQ_DEVICE_H
#define TSQ_DEVICE_H

#include <stdint.h>
#include <string.h>

#include "../../include/tsq.h"

#if defined(__HIPCC__)
#define TSQ_HD __host__ __device__ __forceinline__
#else
#define TSQ_HD inline
#endif
// A value every lane of the wave agrees on (the expression program is the same for all rows): telling the
// compiler so turns the interpreter's switch into scalar branches instead of exec-masked regions for every case.
#if defined(TSQ_JIT)
// run-time specialisation (tsq_expr.hip): the program is a compile-time constant, the op loop unrolls and folds
#define TSQ_UNIFORM(x) ((int)(x))
#define TSQ_JIT_UNROLL _Pragma("unroll")
#elif defined(__HIP_DEVICE_COMPILE__)
#define TSQ_UNIFORM(x) __builtin_amdgcn_readfirstlane((int)(x))
#define TSQ_JIT_UNROLL
#else
#define TSQ_UNIFORM(x) ((int)(x))
#define TSQ_JIT_UNROLL
#endif

// ------------------------------------------------------------------ hashing
// splitmix64 — the synthetic-table generator of SURVEY.md §8(d), also the row-checksum mixer.
TSQ_HD uint64_t tsq_splitmix64(uint64_t x) {
    x += 0x9E3779B97F4A7C15ULL;
    uint64_t z = x;
    z = (z ^ (z >> 30)) * 0xBF58476D1CE4E5B9ULL;
    z = (z ^ (z >> 27)) * 0x94D049BB133111EBULL;
    return z ^ (z >> 31);
}
// Bucket hash of a 64-bit key word.  The reference hashes with FNV-1-64 (executor/hash_table.go:64)
// but the hash value never reaches a result (equality is by bytes, util/codec/codec.go:377), so the
// GPU is free to use a cheaper, better-mixing function.
TSQ_HD uint64_t tsq_mix64(uint64_t k) {
    k ^= k >> 33;
    k *= 0xFF51AFD7ED558CCDULL;
    k ^= k >> 33;
    k *= 0xC4CEB9FE1A85EC53ULL;
    k ^= k >> 33;
    return k;
}
// high 64 bits of a 64x64 multiply: range reduction of a hash to [0, n) without a power-of-two n
TSQ_HD uint64_t tsq_mulhi64(uint64_t a, uint64_t b) {
#if defined(__HIP_DEVICE_COMPILE__)
    return __umul64hi(a, b);
#else
    return (uint64_t)(((unsigned __int128)a * b) >> 64);
#endif
}

// order-independent row checksum: sum and xor over rows of this per-row hash
#define TSQ_ROWHASH_SEED 0x243F6A8885A308D3ULL
#define TSQ_ROWHASH_NULL 0xA5A5A5A55A5A5A5AULL
TSQ_HD uint64_t tsq_rowhash_step(uint64_t h, uint64_t v, uint32_t c) {
    return tsq_splitmix64(h ^ (v + (uint64_t)(c + 1) * 0x9E3779B97F4A7C15ULL));
}

// hash of a var-len cell (string join keys and string group keys: equality is decided by the bytes, so any hash will do)
TSQ_HD uint64_t tsq_hash_bytes(const uint8_t* p, int64_t n) {
    uint64_t w = 0x9E3779B97F4A7C15ULL ^ (uint64_t)n;
    int64_t i = 0;
    for (; i + 8 <= n; i += 8) {
        uint64_t x;
        memcpy(&x, p + i, 8);
        w = tsq_splitmix64(w ^ x);
    }
    uint64_t tail = 0;
    for (int64_t q = i; q < n; q++) tail = (tail << 8) | p[q];
    return tsq_splitmix64(w ^ tail);
}

// one var-len cell copied by ONE lane: eight bytes at a time (global loads and stores take any byte address), then the tail
TSQ_HD void tsq_copy_cell(uint8_t* d, const uint8_t* s, int64_t n) {
    // (d and s never overlap: a cell is copied between two buffers.  No byte loop over memory: every byte load behind a byte store may
    // alias it, so a 7-byte tail was seven dependent round trips — round 6: the tail of a cell of 8 bytes or more is one more 8-byte copy
    // that overlaps the bytes before it, a shorter cell is gathered into a register first)
    if (n >= 8) {
        int64_t i = 0;
        for (; i + 8 <= n; i += 8) {
            uint64_t x;
            memcpy(&x, s + i, 8);
            memcpy(d + i, &x, 8);
        }
        if (i < n) {
            uint64_t x;
            memcpy(&x, s + n - 8, 8);
            memcpy(d + n - 8, &x, 8);
        }
        return;
    }
    uint64_t x = 0;
    for (int64_t i = 0; i < n; i++) x |= (uint64_t)s[i] << (8 * i);
    for (int64_t i = 0; i < n; i++) d[i] = (uint8_t)(x >> (8 * i));
}

// rank of a key for the multi-GPU radix redistribute (tsq_radix_split)
TSQ_HD uint32_t tsq_key_rank(uint64_t kw, uint32_t n_parts) {
    return (uint32_t)(((tsq_mix64(kw) & 0xffffu) * (uint64_t)n_parts) >> 16);
}

// ------------------------------------------------------------------ bit patterns
TSQ_HD double tsq_bits_f64(uint64_t b) {
    double d;
    memcpy(&d, &b, 8);
    return d;
}
TSQ_HD uint64_t tsq_f64_bits(double d) {
    uint64_t b;
    memcpy(&b, &d, 8);
    return b;
}
TSQ_HD float tsq_bits_f32(uint32_t b) {
    float f;
    memcpy(&f, &b, 4);
    return f;
}

// util/chunk/column.go:89-92: bit == 1 => NOT NULL, LSB first; bitmap == nullptr => no NULLs
TSQ_HD bool tsq_is_null(const uint8_t* bm, int64_t i) {
    if (!bm) return false;
    return ((bm[i >> 3] >> (i & 7)) & 1) == 0;
}

// ------------------------------------------------------------------ synthetic tables
TSQ_HD uint64_t tsq_gen_r(uint64_t seed, uint32_t table, uint64_t c, uint64_t i) {
    return tsq_splitmix64(seed ^ ((uint64_t)table << 56) ^ (c << 48) ^ i);
}
TSQ_HD bool tsq_gen_is_null(const tsq_gen_spec& s, uint64_t i) {
    return s.null_pct > 0 && (tsq_gen_r(s.seed, (uint32_t)s.table, 7, i) % 100) < (uint64_t)s.null_pct;
}
TSQ_HD uint64_t tsq_gen_value(const tsq_gen_spec& s, uint64_t i, uint64_t src) {
    switch (s.kind) {
        case TSQ_GEN_SEQ: return i;
        case TSQ_GEN_AFFINE: return (s.a * (i % s.m) + s.b) % s.m;
        case TSQ_GEN_RAND_MOD: return tsq_gen_r(s.seed, (uint32_t)s.table, (uint64_t)s.col, i) % s.m;
        case TSQ_GEN_RAND_F64:
            return tsq_f64_bits((double)(tsq_gen_r(s.seed, (uint32_t)s.table, (uint64_t)s.col, i) >> 11) *
                                (1.0 / 9007199254740992.0));
        case TSQ_GEN_HASH_OF_COL: return tsq_splitmix64(src ^ s.b);
        case TSQ_GEN_ZIPF_OCT: {
            const uint64_t r = tsq_gen_r(s.seed, (uint32_t)s.table, (uint64_t)s.col, i);
            const uint64_t oct = s.a ? (s.a < 63 ? s.a : 63) : 1;  // octaves: a shift of 64 or more is undefined
            const uint64_t lo = 1ull << (r % oct);
            return (lo + (tsq_splitmix64(r) & (lo - 1)) - 1) % s.m;
        }
    }
    return 0;
}

// ------------------------------------------------------------------ join key words
// A join key cell becomes (class flag, 64-bit word) exactly like
// util/codec/codec.go:212-240 encodeHashChunkRowIdx: ints -> raw 8 bytes with flag 8, or 9 when the
// column is UNSIGNED and the value has its top bit set; float32 widened to float64, flag 5.
// Two cells are equal iff flags and words are equal (codec.go:363-382).
#define TSQ_FLAG_INT 8
#define TSQ_FLAG_UINT 9
#define TSQ_FLAG_FLOAT 5
TSQ_HD uint64_t tsq_key_word(const void* data, int32_t type, int64_t row, uint32_t* flag) {
    switch (type) {
        case TSQ_I64: {
            *flag = TSQ_FLAG_INT;
            return ((const uint64_t*)data)[row];
        }
        case TSQ_U64: {
            uint64_t v = ((const uint64_t*)data)[row];
            *flag = (v >> 63) ? TSQ_FLAG_UINT : TSQ_FLAG_INT;
            return v;
        }
        case TSQ_F32: {
            *flag = TSQ_FLAG_FLOAT;
            return tsq_f64_bits((double)((const float*)data)[row]);
        }
        default: {
            *flag = TSQ_FLAG_FLOAT;
            return ((const uint64_t*)data)[row];
        }
    }
}

// ------------------------------------------------------------------ expression interpreter
// One row through one postfix program.  Each opcode restates one builtin*Sig.vecEval* of the
// reference for a single row; see include/tsq.h for the file:line of every opcode.
struct tsq_val {
    int64_t v;   // int64 or the bits of a double
    bool null;
};

// Row sources for the interpreter: the caller decides how (column, logical row) maps to storage.
// tsq_chunk_src  : one chunk, one physical row (chunk.sel already applied by the caller);
// tsq_joined_src : a joined row lhs||rhs living in two chunks (joiner.go:145-150 column order).
struct tsq_colset {  // kernel-argument friendly description of a chunk's columns
    const void* data[TSQ_MAX_COLS];
    const uint8_t* nulls[TSQ_MAX_COLS];
    const int64_t* offs[TSQ_MAX_COLS];  // TSQ_BYTES columns: offsets[n + 1] into data (util/chunk/column.go:28-34)
    int32_t type[TSQ_MAX_COLS];
    int32_t n;
};
// A string VALUE on the evaluation stack is a reference, no bytes move: [63:56] source (column index, or TSQ_STR_POOL = the
// program's constant pool), [55:32] length (< 2^24), [31:0] byte offset into the source's data (< 2^32).
#define TSQ_STR_POOL 0xffu
#define TSQ_STR_MAXLEN 0xffffffu
TSQ_HD uint64_t tsq_str_ref(uint32_t src, uint64_t off, uint64_t len) { return ((uint64_t)src << 56) | (len << 32) | off; }
TSQ_HD uint32_t tsq_str_len(uint64_t h) { return (uint32_t)(h >> 32) & TSQ_STR_MAXLEN; }
// types.CompareString with the binary collation = bytes.Compare (types/compare.go:136-139): -1 / 0 / 1
TSQ_HD int tsq_cmp_bytes(const uint8_t* a, uint32_t la, const uint8_t* b, uint32_t lb) {
    const uint32_t n = la < lb ? la : lb;
    for (uint32_t i = 0; i < n; i++) {
        if (a[i] != b[i]) return a[i] < b[i] ? -1 : 1;
    }
    return la < lb ? -1 : (la == lb ? 0 : 1);
}
// a TSQ_BYTES cell as a string reference; *bad is set when the cell does not fit the reference (TSQ_ERR_UNSUPPORTED)
TSQ_HD uint64_t tsq_cell_str(const tsq_colset& cs, int c, int gc, int64_t row, bool* isnull, bool* bad) {
    *isnull = tsq_is_null(cs.nulls[c], row);
    const int64_t o0 = cs.offs[c][row], o1 = cs.offs[c][row + 1];
    if ((uint64_t)o0 >> 32 || (uint64_t)(o1 - o0) > TSQ_STR_MAXLEN) *bad = true;
    return tsq_str_ref((uint32_t)gc, (uint64_t)o0 & 0xffffffffu, (uint64_t)(o1 - o0) & TSQ_STR_MAXLEN);
}
TSQ_HD tsq_val tsq_cell_int(const tsq_colset& cs, int c, int64_t row) {
    tsq_val r;
    r.null = tsq_is_null(cs.nulls[c], row);
    r.v = ((const int64_t*)cs.data[c])[row];
    return r;
}
TSQ_HD tsq_val tsq_cell_real(const tsq_colset& cs, int c, int64_t row) {
    tsq_val r;
    r.null = tsq_is_null(cs.nulls[c], row);
    if (cs.type[c] == TSQ_F32) r.v = (int64_t)tsq_f64_bits((double)((const float*)cs.data[c])[row]);
    else r.v = ((const int64_t*)cs.data[c])[row];
    return r;
}
// raw 64-bit image of a cell (F32 zero-extended) — what the row checksum and the gather use
TSQ_HD uint64_t tsq_cell_raw(const tsq_colset& cs, int c, int64_t row) {
    if (cs.type[c] == TSQ_F32) return ((const uint32_t*)cs.data[c])[row];
    return ((const uint64_t*)cs.data[c])[row];
}
struct tsq_chunk_src {
    const tsq_colset* cs;
    int64_t row;
    TSQ_HD tsq_val load_int(int c) const { return tsq_cell_int(*cs, c, row); }
    TSQ_HD tsq_val load_real(int c) const { return tsq_cell_real(*cs, c, row); }
    TSQ_HD tsq_val load_str(int c, bool* bad) const {
        tsq_val r;
        r.v = (int64_t)tsq_cell_str(*cs, c, c, row, &r.null, bad);
        return r;
    }
    TSQ_HD const uint8_t* str_base(uint32_t src) const { return (const uint8_t*)cs->data[src]; }
};
struct tsq_joined_src {
    const tsq_colset* left;
    const tsq_colset* right;
    int64_t lrow, rrow;
    TSQ_HD tsq_val load_int(int c) const {
        return c < left->n ? tsq_cell_int(*left, c, lrow) : tsq_cell_int(*right, c - left->n, rrow);
    }
    TSQ_HD tsq_val load_real(int c) const {
        return c < left->n ? tsq_cell_real(*left, c, lrow) : tsq_cell_real(*right, c - left->n, rrow);
    }
    TSQ_HD tsq_val load_str(int c, bool* bad) const {
        tsq_val r;
        r.v = (int64_t)(c < left->n ? tsq_cell_str(*left, c, c, lrow, &r.null, bad) : tsq_cell_str(*right, c - left->n, c, rrow, &r.null, bad));
        return r;
    }
    TSQ_HD const uint8_t* str_base(uint32_t src) const {
        return (const uint8_t*)((int)src < left->n ? left->data[src] : right->data[src - left->n]);
    }
};

#define TSQ_I64MAX 0x7fffffffffffffffLL
#define TSQ_I64MIN (-TSQ_I64MAX - 1)
#define TSQ_U64MAX 0xffffffffffffffffULL
#define TSQ_F64MAX 1.7976931348623157e308

TSQ_HD int64_t tsq_wneg(int64_t v) { return (int64_t)(0 - (uint64_t)v); }
TSQ_HD int64_t tsq_godiv(int64_t a, int64_t b) { return b == -1 ? tsq_wneg(a) : a / b; }
TSQ_HD bool tsq_isinf(double d) { return d > TSQ_F64MAX || d < -TSQ_F64MAX; }

// types/compare.go:44-101
TSQ_HD int tsq_cmp_int(int64_t x, int64_t y, bool ux, bool uy) {
    if (ux && uy) {
        uint64_t a = (uint64_t)x, b = (uint64_t)y;
        return a < b ? -1 : (a == b ? 0 : 1);
    }
    if (ux && !uy) {
        if (y < 0 || (uint64_t)x > (uint64_t)TSQ_I64MAX) return 1;
        return x < y ? -1 : (x == y ? 0 : 1);
    }
    if (!ux && uy) {
        if (x < 0 || (uint64_t)y > (uint64_t)TSQ_I64MAX) return -1;
        return x < y ? -1 : (x == y ? 0 : 1);
    }
    return x < y ? -1 : (x == y ? 0 : 1);
}
TSQ_HD int tsq_cmp_real(double x, double y) { return x < y ? -1 : (x == y ? 0 : 1); }  // compare.go:104
// types/helper.go:28 RoundFloat(f) == 0  <=>  |f| < 0.5 (and NaN is "non zero")
TSQ_HD bool tsq_real_is_zero(double f) {
    double a = f < 0 ? -f : f;
    return a < 0.5;
}

// ------------------------------------------------------------------ types.StrToInt (types/convert.go:223-403)
// The reference trims the string, cuts a valid prefix, may rewrite a float prefix into an integer string (roundIntStr, exponent
// shifts) and hands that to strconv.ParseInt.  Here no string is built: every intermediate string is a sequence of bytes of the
// cell (or a few constant characters) fed one by one into ParseInt's loop, which stops at the first byte that decides the answer.
// Result flags of tsq_str_to_int: one warning of each kind per call at most, and at most one error.
#define TSQ_S2I_TRUNC_WARN 1u  // ErrTruncatedWrongVal appended as a warning (handleTruncateError, types/datum.go:948-957)
#define TSQ_S2I_OVF_WARN 2u    // ErrOverflow "BIGINT" appended as a warning (an exponent beyond 21 digits, convert.go:362-369)
#define TSQ_S2I_ERR_OVF 4u     // returned error ErrOverflow "BIGINT": ParseInt failed (convert.go:226-229)
#define TSQ_S2I_ERR_TRUNC 8u   // returned error ErrTruncatedWrongVal (a truncation under !TruncateAsWarning)

// strconv.ParseInt(s, 10, 64) fed one byte at a time (Go's ParseUint stops at the first uint64 overflow, so a bad byte after it
// is never seen; a bad byte before it is a syntax error)
struct tsq_parseint {
    uint64_t n = 0;
    int64_t k = 0;    // bytes fed
    int st = 0;       // 0 running, 1 syntax error, 2 range error
    bool neg = false, sign = false;
    bool uns = false;  // strconv.ParseUint behind StrToUint's strip of ONE leading '+' (types/convert.go:236-246): no sign is accepted
    TSQ_HD void feed(uint8_t c) {
        if (st) return;
        if (k++ == 0 && (c == '+' || c == '-')) {
            if (uns && c == '-') { st = 1; return; }
            sign = true;
            neg = c == '-';
            return;
        }
        if (c < '0' || c > '9') { st = 1; return; }
        if (n >= TSQ_U64MAX / 10 + 1) { st = 2; return; }
        const uint64_t m = n * 10, m1 = m + (uint64_t)(c - '0');
        if (m1 < m) { st = 2; return; }
        n = m1;
    }
    // value and ok (false: the error ParseInt returns; the value is then 0 or +-MaxInt64 as Go returns it)
    TSQ_HD bool finish(int64_t* v) const {
        if (st == 0 && k - (sign ? 1 : 0) == 0) { *v = 0; return false; }  // "" or a lone sign
        if (st == 1) { *v = 0; return false; }
        if (uns) {  // the uint64 as its bits; a range error is MaxUint64
            *v = (int64_t)(st == 2 ? TSQ_U64MAX : n);
            return st == 0;
        }
        const uint64_t cut = (uint64_t)1 << 63;
        if (st == 2) { *v = neg ? (int64_t)(0 - cut) : (int64_t)(cut - 1); return false; }
        if (!neg && n >= cut) { *v = (int64_t)(cut - 1); return false; }
        if (neg && n > cut) { *v = (int64_t)(0 - cut); return false; }
        *v = neg ? (int64_t)(0 - n) : (int64_t)n;
        return true;
    }
    TSQ_HD void feed_bytes(const uint8_t* b, int64_t from, int64_t to) {
        for (int64_t i = from; i < to && st == 0; i++) feed(b[i]);
    }
    TSQ_HD void feed_zeros(int64_t z) {
        for (int64_t i = 0; i < z && st == 0; i++) feed('0');
    }
};

// unicode.IsSpace as UTF-8 (the White_Space runes): 2-byte U+0085 U+00A0, 3-byte U+1680 U+2000-200A U+2028 U+2029 U+202F U+205F U+3000.
// strings.TrimSpace decodes runes; a space rune is only ever one of these byte sequences, and invalid UTF-8 decodes to U+FFFD (no space).
TSQ_HD bool tsq_space3(uint8_t a, uint8_t b, uint8_t c) {
    if (a == 0xE1) return b == 0x9A && c == 0x80;
    if (a == 0xE3) return b == 0x80 && c == 0x80;
    if (a != 0xE2) return false;
    if (b == 0x80) return (c >= 0x80 && c <= 0x8A) || c == 0xA8 || c == 0xA9 || c == 0xAF;
    return b == 0x81 && c == 0x9F;
}
TSQ_HD bool tsq_ascii_space(uint8_t c) { return c == ' ' || (c >= 9 && c <= 13); }

// roundIntStr(next, body) (convert.go:284-310) fed into `pi`, body(k) = b[k] for k < skip, b[k + 1] from there on (a removed dot).
// Returns false where the reference indexes past a one-character sign (a run-time panic there).
TSQ_HD bool tsq_feed_rounded(tsq_parseint& pi, const uint8_t* b, int64_t len, int64_t skip, bool up) {
    auto body = [&](int64_t k) -> uint8_t { return b[(skip >= 0 && k >= skip) ? k + 1 : k]; };
    if (!up) {
        for (int64_t k = 0; k < len && pi.st == 0; k++) pi.feed(body(k));
        return true;
    }
    int64_t r = len - 1;
    while (r >= 1 && body(r) == '9') r--;
    if (r >= 1) {
        for (int64_t k = 0; k < r && pi.st == 0; k++) pi.feed(body(k));
        pi.feed((uint8_t)(body(r) + 1));
        pi.feed_zeros(len - 1 - r);
        return true;
    }
    const uint8_t c0 = body(0);
    if (c0 == '9') {
        pi.feed('1');
        pi.feed_zeros(len);
    } else if (c0 >= '0' && c0 <= '9') {
        pi.feed((uint8_t)(c0 + 1));
        pi.feed_zeros(len - 1);
    } else {
        if (len < 2) return false;
        pi.feed(c0);
        pi.feed('1');
        pi.feed_zeros(len - 1);
    }
    return true;
}

// types.StrToInt(sc, s[0:n]) with sc's flags in str_ctx (TSQ_STRCTX_*): *v = the value the reference returns (also on error),
// result = TSQ_S2I_* flags.  Reads the leading spaces, the valid prefix plus one byte, and the trailing spaces from the end.
// uns: types.StrToUint instead (convert.go:234-246) — the same prefix, one leading '+' stripped, strconv.ParseUint; *v holds the uint64's
// bits, TSQ_S2I_ERR_OVF stands for ErrOverflow "BIGINT UNSIGNED" (a '-' in front is ParseUint's syntax error: value 0)
TSQ_HD uint32_t tsq_str_to_num(const uint8_t* s, uint32_t n, uint32_t str_ctx, bool uns, int64_t* v) {
    // strings.TrimSpace
    uint32_t lo = 0, hi = n;
    while (lo < hi) {
        const uint8_t c = s[lo];
        if (tsq_ascii_space(c)) lo += 1;
        else if (c == 0xC2 && lo + 1 < hi && (s[lo + 1] == 0x85 || s[lo + 1] == 0xA0)) lo += 2;
        else if (lo + 2 < hi && tsq_space3(c, s[lo + 1], s[lo + 2])) lo += 3;
        else break;
    }
    while (hi > lo) {
        if (tsq_ascii_space(s[hi - 1])) hi -= 1;
        else if (hi - lo >= 2 && s[hi - 2] == 0xC2 && (s[hi - 1] == 0x85 || s[hi - 1] == 0xA0)) hi -= 2;
        else if (hi - lo >= 3 && tsq_space3(s[hi - 3], s[hi - 2], s[hi - 1])) hi -= 3;
        else break;
    }
    const uint8_t* t = s + lo;
    const int64_t len = (int64_t)(hi - lo);
    uint32_t flags = 0;
    bool trunc_err = false;
    auto truncated = [&]() {  // handleTruncateError
        if (str_ctx & TSQ_STRCTX_IGNORE_TRUNCATE) return;
        if (str_ctx & TSQ_STRCTX_TRUNCATE_ERROR) trunc_err = true;
        else flags |= TSQ_S2I_TRUNC_WARN;
    };
    auto done = [&](const tsq_parseint& pi) -> uint32_t {  // StrToInt: ParseInt's failure replaces the prefix's error
        if (!pi.finish(v)) return flags | TSQ_S2I_ERR_OVF;
        return flags | (trunc_err ? TSQ_S2I_ERR_TRUNC : 0u);
    };
    tsq_parseint pi;
    pi.uns = uns;
    if (!(str_ctx & TSQ_STRCTX_NOT_STRICT)) {  // getValidIntPrefix, strict (convert.go:259-281)
        int64_t i = (len > 0 && (t[0] == '+' || t[0] == '-')) ? 1 : 0;
        const int64_t d0 = i;
        while (i < len && t[i] >= '0' && t[i] <= '9') i++;
        const int64_t valid = i > d0 ? i : 0;
        if (valid == 0 || valid != len) truncated();
        if (valid == 0) pi.feed('0');
        else pi.feed_bytes(t, 0, valid);
        return done(pi);
    }
    // getValidFloatPrefix (convert.go:430-478), including its acceptance of a sign at position 1 (eIdx starts at 0)
    if (!(str_ctx & TSQ_STRCTX_EMPTY_NOT_ZERO) && len == 0) { *v = 0; return 0; }
    bool saw_dot = false, saw_digit = false;
    int64_t valid = 0, eidx = 0, dot = -1;
    for (int64_t i = 0; i < len; i++) {
        const uint8_t c = t[i];
        if (c == '+' || c == '-') {
            if (i != 0 && i != eidx + 1) break;
        } else if (c == '.') {
            if (saw_dot || eidx > 0) break;
            saw_dot = true;
            dot = i;
            if (saw_digit) valid = i + 1;
        } else if (c == 'e' || c == 'E') {
            if (!saw_digit || eidx != 0) break;
            eidx = i;
        } else if (c < '0' || c > '9') {
            break;
        } else {
            saw_digit = true;
            valid = i + 1;
        }
    }
    if (valid == 0 || valid != len) truncated();
    if (valid == 0) { *v = 0; return flags | (trunc_err ? TSQ_S2I_ERR_TRUNC : 0u); }  // "0", whichever way it goes
    if (trunc_err) {  // getValidIntPrefix returns the float prefix unconverted
        pi.feed_bytes(t, 0, valid);
        return done(pi);
    }
    // floatStrToIntStr(prefix) (convert.go:318-403); D, E = the dot and the exponent inside the prefix
    const int64_t D = dot >= 0 && dot < valid ? dot : -1, E = eidx > 0 && eidx < valid ? eidx : -1;
    if (E < 0) {
        if (D < 0) {
            pi.feed_bytes(t, 0, valid);
            return done(pi);
        }
        const int64_t sg = (t[0] == '-' || t[0] == '+') ? 1 : 0, di = D - sg;  // digits = prefix[sg:], dotIdx within it
        const bool up = valid > D + 1 && t[D + 1] >= '5';
        if (di == 0) {  // intStr "0", rounded to "1" by a digit >= 5 after the dot; "-" in front of a "1"
            if (up && t[0] == '-') pi.feed('-');
            pi.feed(up ? '1' : '0');
            return done(pi);
        }
        // "-" goes in front unless the rounded string is "0"
        if (t[0] == '-' && !(di == 1 && t[sg] == '0' && !up)) pi.feed('-');
        if (!tsq_feed_rounded(pi, t + sg, di, -1, up)) { *v = 0; return flags | TSQ_S2I_ERR_OVF; }
        return done(pi);
    }
    // with an exponent: digits = prefix[:E] without its dot (a sign stays in it and counts in intCnt)
    const int64_t ndig = D >= 0 ? E - 1 : E;
    auto digit = [&](int64_t k) -> uint8_t { return t[(D >= 0 && k >= D) ? k + 1 : k]; };
    tsq_parseint ex;  // strconv.Atoi(prefix[E + 1:]) = ParseInt: "[sign]digits", so only a range error is possible
    ex.feed_bytes(t, E + 1, valid);
    int64_t exp;
    if (!ex.finish(&exp)) {  // getValidIntPrefix returns the prefix, 'e' and all: ParseInt fails (a syntax error, or a range error first)
        pi.feed_bytes(t, 0, valid);
        return done(pi);
    }
    const int64_t icnt = (int64_t)((uint64_t)(D >= 0 ? D : E) + (uint64_t)exp);  // Go's int addition wraps
    if (exp >= 0 && (icnt > 21 || icnt < 0)) {
        flags |= TSQ_S2I_OVF_WARN;  // AppendWarning, whatever the truncate flags say; the mantissa goes to ParseInt
        pi.feed_bytes(t, 0, E);
        return done(pi);
    }
    if (icnt <= 0) {
        const bool up = icnt == 0 && ndig > 0 && digit(0) >= '5' && digit(0) <= '9';
        *v = up ? 1 : 0;
        return flags;
    }
    if (icnt == 1 && (digit(0) == '-' || digit(0) == '+')) {
        const bool up = ndig > 1 && digit(1) >= '5';
        *v = up ? (digit(0) == '-' ? -1 : 1) : 0;
        if (uns && *v < 0) { *v = 0; return flags | TSQ_S2I_ERR_OVF; }  // ParseUint("-1")
        return flags;
    }
    if (icnt <= ndig) {
        const bool up = icnt < ndig && digit(icnt) >= '5';
        if (!tsq_feed_rounded(pi, t, icnt, D, up)) { *v = 0; return flags | TSQ_S2I_ERR_OVF; }
        return done(pi);
    }
    for (int64_t k = 0; k < ndig && pi.st == 0; k++) pi.feed(digit(k));
    pi.feed_zeros(icnt - ndig);
    return done(pi);
}

TSQ_HD uint32_t tsq_str_to_int(const uint8_t* s, uint32_t n, uint32_t str_ctx, int64_t* v) { return tsq_str_to_num(s, n, str_ctx, false, v); }
TSQ_HD uint32_t tsq_str_to_uint(const uint8_t* s, uint32_t n, uint32_t str_ctx, uint64_t* v) {
    int64_t x = 0;
    const uint32_t f = tsq_str_to_num(s, n, str_ctx, true, &x);
    *v = (uint64_t)x;
    return f;
}

// Evaluates `p` for one row.  Returns TSQ_OK or an overflow status; *err_node receives the
// postfix index of the offending node.  *div0 is incremented per x/0 (errors.go:65-77 warning).
template <class Src>
TSQ_HD tsq_status tsq_eval_row(const tsq_expr_prog& p, const Src& src, tsq_val* out, int* err_node, int* div0) {
    // Evaluation stack with the top two entries cached in registers (r0 = top, r1 = below it); only deeper entries
    // touch `mem`, a dynamically indexed array that the GPU compiler has to place in scratch memory.  With the whole
    // stack in that array a 5-node expression ran at 7 % of the HBM roofline (profiles/r01_kernels.txt).
    tsq_val mem[TSQ_EXPR_MAX_STACK];
    tsq_val r0, r1;
    r0.v = r1.v = 0;
    r0.null = r1.null = true;
    int sp = 0;
    auto push = [&](const tsq_val& x) {
        if (sp >= 2) mem[sp - 2] = r1;
        r1 = r0;
        r0 = x;
        sp++;
    };
    auto pop = [&]() -> tsq_val {
        const tsq_val x = r0;
        r0 = r1;
        if (sp >= 3) r1 = mem[sp - 3];
        sp--;
        return x;
    };
    const int n_ops = TSQ_UNIFORM(p.n_ops);
    TSQ_JIT_UNROLL
    for (int k = 0; k < n_ops; k++) {
        tsq_expr_op op;
        op.opcode = TSQ_UNIFORM(p.ops[k].opcode);
        op.flags = TSQ_UNIFORM(p.ops[k].flags);
        op.arg = TSQ_UNIFORM(p.ops[k].arg);
        op.aux = (decltype(op.aux))TSQ_UNIFORM(p.ops[k].aux);
        const bool ul = op.flags & TSQ_F_LHS_UNSIGNED, ur = op.flags & TSQ_F_RHS_UNSIGNED;
        *err_node = k;
        switch (op.opcode) {
            case TSQ_OP_COL_INT: push(src.load_int(op.arg)); break;
            case TSQ_OP_COL_REAL: push(src.load_real(op.arg)); break;
            case TSQ_OP_CONST_INT:
            case TSQ_OP_CONST_REAL: { tsq_val c; c.v = p.consts[op.arg]; c.null = false; push(c); break; }
            case TSQ_OP_CONST_NULL_INT:
            case TSQ_OP_CONST_NULL_REAL: { tsq_val c; c.v = 0; c.null = true; push(c); break; }
            case TSQ_OP_PLUS_REAL:
            case TSQ_OP_MINUS_REAL:
            case TSQ_OP_MUL_REAL:
            case TSQ_OP_DIV_REAL: {
                tsq_val b = pop();
                tsq_val& a = r0;
                a.null = a.null || b.null;
                if (a.null) break;
                double x = tsq_bits_f64((uint64_t)a.v), y = tsq_bits_f64((uint64_t)b.v), r;
                if (op.opcode == TSQ_OP_PLUS_REAL) {
                    if ((x > 0 && y > TSQ_F64MAX - x) || (x < 0 && y < -TSQ_F64MAX - x)) return TSQ_ERR_OVERFLOW_DOUBLE;
                    r = x + y;
                } else if (op.opcode == TSQ_OP_MINUS_REAL) {
                    if ((x > 0 && -y > TSQ_F64MAX - x) || (x < 0 && -y < -TSQ_F64MAX - x)) return TSQ_ERR_OVERFLOW_DOUBLE;
                    r = x - y;
                } else if (op.opcode == TSQ_OP_MUL_REAL) {
                    r = x * y;
                    if (tsq_isinf(r)) return TSQ_ERR_OVERFLOW_DOUBLE;
                } else {
                    if (y == 0) {
                        (*div0)++;
                        a.null = true;
                        break;
                    }
                    r = x / y;
                    if (tsq_isinf(r)) return TSQ_ERR_OVERFLOW_DOUBLE;
                }
                a.v = (int64_t)tsq_f64_bits(r);
                break;
            }
            case TSQ_OP_PLUS_INT: {
                tsq_val b = pop();
                tsq_val& a = r0;
                a.null = a.null || b.null;
                if (a.null) break;
                int64_t lh = a.v, rh = b.v;
                if (ul && ur) {
                    if ((uint64_t)lh > TSQ_U64MAX - (uint64_t)rh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                } else if (ul && !ur) {  // plusUS incl. the reference's lh-vs-lh check (:454)
                    if (rh < 0 && (uint64_t)tsq_wneg(rh) > (uint64_t)lh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                    if (rh > 0 && (uint64_t)lh > TSQ_U64MAX - (uint64_t)lh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                } else if (!ul && ur) {
                    if (lh < 0 && (uint64_t)tsq_wneg(lh) > (uint64_t)rh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                    if (lh > 0 && (uint64_t)rh > TSQ_U64MAX - (uint64_t)lh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                } else {
                    if ((lh > 0 && rh > TSQ_I64MAX - lh) || (lh < 0 && rh < TSQ_I64MIN - lh)) return TSQ_ERR_OVERFLOW_BIGINT;
                }
                a.v = (int64_t)((uint64_t)lh + (uint64_t)rh);
                break;
            }
            case TSQ_OP_MINUS_INT: {
                tsq_val b = pop();
                tsq_val& a = r0;
                a.null = a.null || b.null;
                if (a.null) break;
                const bool force = op.flags & TSQ_F_FORCE_SIGNED;
                int64_t lh = a.v, rh = b.v;
                const int64_t nrh = tsq_wneg(rh);
                const bool ss_over = (lh > 0 && nrh > TSQ_I64MAX - lh) || (lh < 0 && nrh < TSQ_I64MIN - lh);
                if (force && ul && ur) {
                    if (lh < 0 || rh < 0) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                    if (ss_over) return TSQ_ERR_OVERFLOW_BIGINT;
                } else if (force && ul && !ur) {
                    if (lh < 0) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                    if (ss_over) return TSQ_ERR_OVERFLOW_BIGINT;
                } else if (force && !ul && ur) {
                    if (rh < 0) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                    if (ss_over) return TSQ_ERR_OVERFLOW_BIGINT;
                } else if (!force && ul && ur) {
                    if ((uint64_t)lh < (uint64_t)rh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                } else if (!force && ul && !ur) {
                    if (rh >= 0 && (uint64_t)lh < (uint64_t)rh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                    if (rh < 0 && (uint64_t)lh > TSQ_U64MAX - (uint64_t)nrh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                } else if (!force && !ul && ur) {
                    if (((uint64_t)lh - (uint64_t)TSQ_I64MIN) < (uint64_t)rh) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                } else {
                    if (ss_over) return TSQ_ERR_OVERFLOW_BIGINT;
                }
                a.v = (int64_t)((uint64_t)lh - (uint64_t)rh);
                break;
            }
            case TSQ_OP_MUL_INT: {
                tsq_val b = pop();
                tsq_val& a = r0;
                a.null = a.null || b.null;
                if (a.null) break;
                int64_t x = a.v, y = b.v;
                int64_t tmp = (int64_t)((uint64_t)x * (uint64_t)y);
                if (x != 0 && tsq_godiv(tmp, x) != y) return TSQ_ERR_OVERFLOW_BIGINT;
                a.v = tmp;
                break;
            }
            case TSQ_OP_MUL_INT_UNSIGNED: {
                tsq_val b = pop();
                tsq_val& a = r0;
                a.null = a.null || b.null;
                if (a.null) break;
                uint64_t x = (uint64_t)a.v, y = (uint64_t)b.v, res = x * y;
                if (x != 0 && res / x != y) return TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED;
                a.v = (int64_t)res;
                break;
            }
            case TSQ_OP_LT_INT: case TSQ_OP_LE_INT: case TSQ_OP_GT_INT:
            case TSQ_OP_GE_INT: case TSQ_OP_EQ_INT: case TSQ_OP_NE_INT:
            case TSQ_OP_LT_REAL: case TSQ_OP_LE_REAL: case TSQ_OP_GT_REAL:
            case TSQ_OP_GE_REAL: case TSQ_OP_EQ_REAL: case TSQ_OP_NE_REAL: {
                tsq_val b = pop();
                tsq_val& a = r0;
                a.null = a.null || b.null;
                if (a.null) { a.v = 0; break; }
                const bool isreal = op.opcode >= TSQ_OP_LT_REAL;
                const int rel = isreal ? op.opcode - TSQ_OP_LT_REAL : op.opcode - TSQ_OP_LT_INT;
                int c = isreal ? tsq_cmp_real(tsq_bits_f64((uint64_t)a.v), tsq_bits_f64((uint64_t)b.v))
                               : tsq_cmp_int(a.v, b.v, ul, ur);
                bool v = rel == 0 ? c < 0 : rel == 1 ? c <= 0 : rel == 2 ? c > 0 : rel == 3 ? c >= 0 : rel == 4 ? c == 0 : c != 0;
                a.v = v ? 1 : 0;
                break;
            }
            case TSQ_OP_LOGIC_AND: {
                tsq_val b = pop();
                tsq_val& a = r0;
                if (!a.null && a.v == 0) break;
                if (!b.null && b.v == 0) { a.v = 0; a.null = false; break; }
                if (a.null || b.null) { a.null = true; break; }
                a.v = 1;
                break;
            }
            case TSQ_OP_LOGIC_OR: {
                tsq_val b = pop();
                tsq_val& a = r0;
                if ((!a.null && a.v != 0) || (!b.null && b.v != 0)) { a.v = 1; a.null = false; }
                else if (a.null || b.null) a.null = true;
                else { a.v = 0; a.null = false; }
                break;
            }
            case TSQ_OP_NOT_INT: {
                tsq_val& a = r0;
                if (!a.null) a.v = a.v == 0 ? 1 : 0;
                break;
            }
            case TSQ_OP_NOT_REAL: {
                tsq_val& a = r0;
                if (!a.null) a.v = tsq_bits_f64((uint64_t)a.v) == 0 ? 1 : 0;
                else a.v = 0;
                break;
            }
            case TSQ_OP_NEG_INT: {
                tsq_val& a = r0;
                if (a.null) break;
                if (ul) {
                    if ((uint64_t)a.v > ((uint64_t)1 << 63)) return TSQ_ERR_OVERFLOW_BIGINT;
                } else if (a.v == TSQ_I64MIN) return TSQ_ERR_OVERFLOW_BIGINT;
                a.v = tsq_wneg(a.v);
                break;
            }
            case TSQ_OP_NEG_REAL: {
                tsq_val& a = r0;
                a.v = (int64_t)tsq_f64_bits(-tsq_bits_f64((uint64_t)a.v));
                break;
            }
            case TSQ_OP_ISNULL_INT:
            case TSQ_OP_ISNULL_REAL: {
                tsq_val& a = r0;
                a.v = a.null ? 1 : 0;
                a.null = false;
                break;
            }
            case TSQ_OP_IFNULL_INT:
            case TSQ_OP_IFNULL_REAL: {
                tsq_val b = pop();
                tsq_val& a = r0;
                if (a.null && !b.null) a = b;
                break;
            }
            case TSQ_OP_IF_INT:
            case TSQ_OP_IF_REAL: {
                tsq_val c2 = pop();
                tsq_val c1 = pop();
                tsq_val& c0 = r0;
                if (c0.null || c0.v == 0) c0 = c2;
                else c0 = c1;
                break;
            }
            case TSQ_OP_IN_INT:
            case TSQ_OP_IN_REAL: {
                const int nitems = op.arg;
                // rare and wide: spill the cached entries so that the whole stack is addressable
                if (sp >= 2) mem[sp - 2] = r1;
                mem[sp - 1] = r0;
                tsq_val* st = mem;
                const tsq_val x = st[sp - nitems - 1];
                bool hasNull = false, found = false;
                for (int j = 0; j < nitems; j++) {
                    const tsq_val it = st[sp - nitems + j];
                    if (it.null || x.null) { hasNull = true; continue; }
                    bool eq;
                    if (op.opcode == TSQ_OP_IN_REAL) eq = tsq_cmp_real(tsq_bits_f64((uint64_t)x.v), tsq_bits_f64((uint64_t)it.v)) == 0;
                    else {
                        const bool uj = (op.aux >> j) & 1;
                        if (ul == uj) eq = it.v == x.v;
                        else if (!ul && uj) eq = x.v >= 0 && it.v == x.v;
                        else eq = it.v >= 0 && it.v == x.v;
                    }
                    found = found || eq;
                }
                sp -= nitems;
                r0.v = found ? 1 : 0;
                r0.null = found ? false : hasNull;
                if (sp >= 2) r1 = mem[sp - 2];
                break;
            }
            case TSQ_OP_COL_STR: {
                bool bad = false;
                const tsq_val x = src.load_str(op.arg, &bad);
                if (bad) return TSQ_ERR_UNSUPPORTED;  // a cell beyond 4 GB of column data or longer than 16 MB
                push(x);
                break;
            }
            case TSQ_OP_CONST_STR: {
                tsq_val c;
                const uint64_t ol = (uint64_t)p.consts[op.arg];
                c.v = (int64_t)tsq_str_ref(TSQ_STR_POOL, ol >> 32, ol & TSQ_STR_MAXLEN);
                c.null = false;
                push(c);
                break;
            }
            case TSQ_OP_CONST_NULL_STR: { tsq_val c; c.v = 0; c.null = true; push(c); break; }
            case TSQ_OP_LT_STR: case TSQ_OP_LE_STR: case TSQ_OP_GT_STR:
            case TSQ_OP_GE_STR: case TSQ_OP_EQ_STR: case TSQ_OP_NE_STR:
            case TSQ_OP_STRCMP: {
                tsq_val b = pop();
                tsq_val& a = r0;
                a.null = a.null || b.null;
                if (a.null) { a.v = 0; break; }
                const uint64_t ha = (uint64_t)a.v, hb = (uint64_t)b.v;
                const uint32_t sa = (uint32_t)(ha >> 56), sb = (uint32_t)(hb >> 56);
                const uint8_t* pa = (sa == TSQ_STR_POOL ? (const uint8_t*)p.str_pool : src.str_base(sa)) + (uint32_t)ha;
                const uint8_t* pb = (sb == TSQ_STR_POOL ? (const uint8_t*)p.str_pool : src.str_base(sb)) + (uint32_t)hb;
                const int c = tsq_cmp_bytes(pa, tsq_str_len(ha), pb, tsq_str_len(hb));
                if (op.opcode == TSQ_OP_STRCMP) { a.v = c; break; }
                const int rel = op.opcode - TSQ_OP_LT_STR;
                const bool v = rel == 0 ? c < 0 : rel == 1 ? c <= 0 : rel == 2 ? c > 0 : rel == 3 ? c >= 0 : rel == 4 ? c == 0 : c != 0;
                a.v = v ? 1 : 0;
                break;
            }
            case TSQ_OP_LENGTH: {
                tsq_val& a = r0;
                a.v = a.null ? 0 : (int64_t)tsq_str_len((uint64_t)a.v);
                break;
            }
            case TSQ_OP_ISNULL_STR: {
                tsq_val& a = r0;
                a.v = a.null ? 1 : 0;
                a.null = false;
                break;
            }
            case TSQ_OP_IFNULL_STR: {
                tsq_val b = pop();
                tsq_val& a = r0;
                if (a.null && !b.null) a = b;
                break;
            }
            case TSQ_OP_IF_STR: {
                tsq_val c2 = pop();
                tsq_val c1 = pop();
                tsq_val& c0 = r0;
                if (c0.null || c0.v == 0) c0 = c2;
                else c0 = c1;
                break;
            }
            case TSQ_OP_IN_STR: {
                const int nitems = op.arg;
                if (sp >= 2) mem[sp - 2] = r1;
                mem[sp - 1] = r0;
                tsq_val* st = mem;
                const tsq_val x = st[sp - nitems - 1];
                bool hasNull = false, found = false;
                for (int j = 0; j < nitems; j++) {
                    const tsq_val it = st[sp - nitems + j];
                    if (it.null || x.null) { hasNull = true; continue; }
                    const uint64_t ha = (uint64_t)x.v, hb = (uint64_t)it.v;
                    const uint32_t sa = (uint32_t)(ha >> 56), sb = (uint32_t)(hb >> 56);
                    const uint8_t* pa = (sa == TSQ_STR_POOL ? (const uint8_t*)p.str_pool : src.str_base(sa)) + (uint32_t)ha;
                    const uint8_t* pb = (sb == TSQ_STR_POOL ? (const uint8_t*)p.str_pool : src.str_base(sb)) + (uint32_t)hb;
                    found = found || tsq_cmp_bytes(pa, tsq_str_len(ha), pb, tsq_str_len(hb)) == 0;
                }
                sp -= nitems;
                r0.v = found ? 1 : 0;
                r0.null = found ? false : hasNull;
                if (sp >= 2) r1 = mem[sp - 2];
                break;
            }
            default: return TSQ_ERR_INVALID;
        }
    }
    *out = r0;
    if (out->null) out->v = 0;
    return TSQ_OK;
}

// expression.VecEvalBool for one row (expression/expression.go:205-279): conjuncts are evaluated in
// order and only while the row is still alive; an Int-typed NULL keeps the row alive but marks it
// (`nulls`), a Real-typed NULL drops it; truthiness per toBool (:281-326).
// String-valued conjuncts (result_type TSQ_BYTES, ABI 8) take the ETString arm of toBool: a NULL drops the row, any other value
// is types.StrToInt'ed under the program's str_ctx and the row lives iff the value != 0.  That arm is compiled only for a Sink
// with ON = true, which hears about every non-NULL string row a conjunct saw: sink->str_row(conjunct, TSQ_S2I_* flags).  A status
// other than TSQ_OK it returns is the row's error (the joins: any conversion error fails them); tsq_filter_eval's sink returns
// TSQ_OK and applies the last-row rule itself.  tsq_no_str_sink (the numeric kernels) leaves the function exactly as it was.
struct tsq_no_str_sink {
    static constexpr bool ON = false;
    TSQ_HD tsq_status str_row(int, uint32_t) { return TSQ_OK; }
};
template <class Src, class Sink = tsq_no_str_sink>
TSQ_HD tsq_status tsq_filter_row(const tsq_expr_prog* progs, int n_progs, const Src& src, bool* selected,
                                 bool* isnull, int* err_conj, int* err_node, int* div0, Sink* sink = nullptr) {
    bool nulls = false, alive = true;
    TSQ_JIT_UNROLL
    for (int e = 0; e < n_progs && alive; e++) {
        tsq_val v;
        *err_conj = e;
        tsq_status s = tsq_eval_row(progs[e], src, &v, err_node, div0);
        if (s != TSQ_OK) return s;
        if (Sink::ON && TSQ_UNIFORM(progs[e].result_type) == TSQ_BYTES) {
            if (v.null) {
                alive = false;
                continue;
            }
            const uint64_t h = (uint64_t)v.v;
            const uint32_t sc = (uint32_t)(h >> 56);
            const uint8_t* b = (sc == TSQ_STR_POOL ? (const uint8_t*)progs[e].str_pool : src.str_base(sc)) + (uint32_t)h;
            int64_t x = 0;
            const tsq_status q = sink->str_row(e, tsq_str_to_int(b, tsq_str_len(h), (uint32_t)TSQ_UNIFORM(progs[e].str_ctx), &x));
            if (q != TSQ_OK) return q;
            if (x == 0) alive = false;
            continue;
        }
        const bool isint = progs[e].result_type != TSQ_F64;
        if (v.null) {
            if (isint) nulls = true;
            else alive = false;
        } else if (isint ? (v.v == 0) : tsq_real_is_zero(tsq_bits_f64((uint64_t)v.v))) {
            alive = false;
        }
    }
    *selected = alive && !nulls;
    *isnull = nulls;
    return TSQ_OK;
}

// Counter words of the filter kernels (tsq_expr.hip) for the string conjuncts, 4 per conjunct from TSQ_STRCNT_BASE: the largest
// row + 1 of a non-NULL row that reached it (atomicMax), the largest (row + 1) << 2 | kind of such a row that raised an error
// (kind 1 ErrOverflow, 2 ErrTruncatedWrongVal), and the two warning counts.  The conjunct fails iff the two rows are the same.
#define TSQ_STRCNT_BASE 4
#define TSQ_STRCNT_WORDS (TSQ_STRCNT_BASE + 4 * 16)
#if defined(__HIPCC__) || defined(TSQ_JIT)
// per lane: a lane's rows come in increasing order, so the last row it saw is its largest.  N conjuncts (compile-time in the JIT:
// registers; the interpreter's 16 live in scratch)
template <int N>
struct tsq_str_lane_sink {
    static constexpr bool ON = true;
    uint64_t row1 = 0;
    uint64_t reached[N], err[N];
    uint32_t trunc[N], ovf[N];
    __device__ tsq_str_lane_sink() {
#pragma unroll
        for (int e = 0; e < N; e++) reached[e] = err[e] = 0, trunc[e] = ovf[e] = 0;
    }
    __device__ tsq_status str_row(int e, uint32_t f) {
        reached[e] = row1;
        if (f & (TSQ_S2I_ERR_OVF | TSQ_S2I_ERR_TRUNC)) err[e] = (row1 << 2) | ((f & TSQ_S2I_ERR_OVF) ? 1u : 2u);
        trunc[e] += f & TSQ_S2I_TRUNC_WARN;
        ovf[e] += (f & TSQ_S2I_OVF_WARN) >> 1;
        return TSQ_OK;
    }
    // whole wave (every lane must be here): reduced over the wave, one atomic per word and wave
    __device__ void flush(unsigned long long* counters, const tsq_expr_prog* progs, int n_progs) {
        TSQ_JIT_UNROLL
        for (int e = 0; e < N && e < n_progs; e++) {
            if (TSQ_UNIFORM(progs[e].result_type) != TSQ_BYTES) continue;
            unsigned long long r = reached[e], x = err[e], t = trunc[e], o = ovf[e];
            for (int s = 32; s >= 1; s >>= 1) {
                const unsigned long long r2 = __shfl_xor(r, s), x2 = __shfl_xor(x, s);
                r = r2 > r ? r2 : r;
                x = x2 > x ? x2 : x;
                t += __shfl_xor(t, s);
                o += __shfl_xor(o, s);
            }
            if ((threadIdx.x & 63) == 0) {
                unsigned long long* c = counters + TSQ_STRCNT_BASE + 4 * e;
                if (r) atomicMax(c, r);
                if (x) atomicMax(c + 1, x);
                if (t) atomicAdd(c + 2, t);
                if (o) atomicAdd(c + 3, o);
            }
        }
    }
};
// The joins' conditions and outer filters: the reference's "last row" depends on its chunk boundaries and on the order of a probe
// row's candidates in the hash chain, neither of which the library reproduces; so a join fails with the conversion error iff ANY
// row or pair it evaluated raised one, through the ordinary error word.  Warnings: one device atomic per warning
// into warn[0] (truncated) / warn[1] (overflow) — nullptr: not counted by this pass (the emit pass walks the rows the count pass
// counted already).
struct tsq_any_str_sink {
    static constexpr bool ON = true;
    unsigned long long* warn;
    __device__ tsq_status str_row(int, uint32_t f) {
        if (warn) {
            if (f & TSQ_S2I_TRUNC_WARN) atomicAdd(warn, 1ull);
            if (f & TSQ_S2I_OVF_WARN) atomicAdd(warn + 1, 1ull);
        }
        return (f & TSQ_S2I_ERR_OVF) ? TSQ_ERR_OVERFLOW_BIGINT : ((f & TSQ_S2I_ERR_TRUNC) ? TSQ_ERR_TRUNCATED_WRONG_VALUE : TSQ_OK);
    }
};
#endif

// error word for "first offending node, then first offending row" semantics of the vectorized
// evaluator: smaller == earlier in the reference's evaluation order.  atomicMin'ed by kernels.
//   [63:58] conjunct  [57:52] node  [51:4] row  [3:0] status
#define TSQ_ERRWORD_NONE 0xffffffffffffffffULL
TSQ_HD uint64_t tsq_errword(int conj, int node, uint64_t row, tsq_status st) {
    return ((uint64_t)conj << 58) | ((uint64_t)node << 52) | ((row & 0xffffffffffffULL) << 4) | (uint64_t)(st & 15);
}

// Static validation of a program (stack discipline, value kinds, indices, result type): host side, at compile.
// col_types (optional, n_cols entries) lets the column leaves be checked against the schema.
inline tsq_status tsq_validate_prog(const tsq_expr_prog& p, int32_t n_cols, const char** why, const int32_t* col_types = nullptr) {
    if (p.n_ops <= 0 || p.n_ops > TSQ_EXPR_MAX_OPS) { *why = "n_ops out of range"; return TSQ_ERR_INVALID; }
    if (p.str_ctx & ~TSQ_STRCTX_ALL) { *why = "str_ctx has an unknown bit"; return TSQ_ERR_INVALID; }
    if (p.n_consts < 0 || p.n_consts > TSQ_EXPR_MAX_CONSTS) { *why = "n_consts out of range"; return TSQ_ERR_INVALID; }
    if (p.n_str_bytes < 0 || p.n_str_bytes > TSQ_EXPR_STR_POOL) { *why = "string pool size out of range"; return TSQ_ERR_INVALID; }
    bool is_str[TSQ_EXPR_MAX_STACK + 1];  // kind of every stack entry: string reference or number
    int sp = 0;
    for (int k = 0; k < p.n_ops; k++) {
        const tsq_expr_op& op = p.ops[k];
        int pop = 0;
        bool res_str = false;
        int str_args = -1;  // -1: all popped values must be numbers; otherwise a bit mask of the popped entries (bit 0 = deepest) that must be strings
        switch (op.opcode) {
            case TSQ_OP_COL_INT: case TSQ_OP_COL_REAL: case TSQ_OP_COL_STR:
                if (n_cols >= 0 && op.arg >= n_cols) { *why = "column index out of range"; return TSQ_ERR_INVALID; }
                if (col_types && ((col_types[op.arg] == TSQ_BYTES) != (op.opcode == TSQ_OP_COL_STR))) { *why = "column leaf does not match the column type"; return TSQ_ERR_INVALID; }
                res_str = op.opcode == TSQ_OP_COL_STR;
                break;
            case TSQ_OP_CONST_INT: case TSQ_OP_CONST_REAL:
                if (op.arg >= p.n_consts) { *why = "const index out of range"; return TSQ_ERR_INVALID; }
                break;
            case TSQ_OP_CONST_STR: {
                if (op.arg >= p.n_consts) { *why = "const index out of range"; return TSQ_ERR_INVALID; }
                const uint64_t ol = (uint64_t)p.consts[op.arg];
                if ((ol >> 32) + (ol & 0xffffffffu) > (uint64_t)p.n_str_bytes) { *why = "string constant outside the pool"; return TSQ_ERR_INVALID; }
                res_str = true;
                break;
            }
            case TSQ_OP_CONST_NULL_INT: case TSQ_OP_CONST_NULL_REAL: break;
            case TSQ_OP_CONST_NULL_STR: res_str = true; break;
            case TSQ_OP_PLUS_REAL: case TSQ_OP_MINUS_REAL: case TSQ_OP_MUL_REAL: case TSQ_OP_DIV_REAL:
            case TSQ_OP_PLUS_INT: case TSQ_OP_MINUS_INT: case TSQ_OP_MUL_INT: case TSQ_OP_MUL_INT_UNSIGNED:
            case TSQ_OP_LT_INT: case TSQ_OP_LE_INT: case TSQ_OP_GT_INT: case TSQ_OP_GE_INT:
            case TSQ_OP_EQ_INT: case TSQ_OP_NE_INT: case TSQ_OP_LT_REAL: case TSQ_OP_LE_REAL:
            case TSQ_OP_GT_REAL: case TSQ_OP_GE_REAL: case TSQ_OP_EQ_REAL: case TSQ_OP_NE_REAL:
            case TSQ_OP_LOGIC_AND: case TSQ_OP_LOGIC_OR: case TSQ_OP_IFNULL_INT: case TSQ_OP_IFNULL_REAL:
                pop = 2;
                break;
            case TSQ_OP_LT_STR: case TSQ_OP_LE_STR: case TSQ_OP_GT_STR: case TSQ_OP_GE_STR:
            case TSQ_OP_EQ_STR: case TSQ_OP_NE_STR: case TSQ_OP_STRCMP:
                pop = 2;
                str_args = 3;
                break;
            case TSQ_OP_IFNULL_STR:
                pop = 2;
                str_args = 3;
                res_str = true;
                break;
            case TSQ_OP_NOT_INT: case TSQ_OP_NOT_REAL: case TSQ_OP_NEG_INT: case TSQ_OP_NEG_REAL:
            case TSQ_OP_ISNULL_INT: case TSQ_OP_ISNULL_REAL:
                pop = 1;
                break;
            case TSQ_OP_LENGTH: case TSQ_OP_ISNULL_STR:
                pop = 1;
                str_args = 1;
                break;
            case TSQ_OP_IF_INT: case TSQ_OP_IF_REAL: pop = 3; break;
            case TSQ_OP_IF_STR:
                pop = 3;
                str_args = 6;  // cond is a number, both values are strings
                res_str = true;
                break;
            case TSQ_OP_IN_INT: case TSQ_OP_IN_REAL: case TSQ_OP_IN_STR:
                if (op.arg < 1 || op.arg > 31) { *why = "IN list size out of range"; return TSQ_ERR_INVALID; }
                pop = op.arg + 1;
                if (op.opcode == TSQ_OP_IN_STR) str_args = -2;  // every popped value is a string
                break;
            default: *why = "unknown opcode"; return TSQ_ERR_UNSUPPORTED;
        }
        if (sp < pop) { *why = "stack underflow"; return TSQ_ERR_INVALID; }
        for (int q = 0; q < pop; q++) {
            const bool want = str_args == -2 ? true : (str_args < 0 ? false : ((str_args >> q) & 1) != 0);
            if (is_str[sp - pop + q] != want) { *why = "operand kind (string / number) does not match the opcode"; return TSQ_ERR_INVALID; }
        }
        sp = sp - pop + 1;
        if (sp > TSQ_EXPR_MAX_STACK) { *why = "expression too deep"; return TSQ_ERR_UNSUPPORTED; }
        is_str[sp - 1] = res_str;
    }
    if (sp != 1) { *why = "program leaves stack depth != 1"; return TSQ_ERR_INVALID; }
    // a string-valued root (IF / IFNULL of strings, a string column, a string constant) is declared by result_type TSQ_BYTES and
    // evaluated by tsq_expr_eval_str only; conditions and filters need an Int or Real root
    // A string-valued root declared as a number is a plan the numeric evaluators cannot take — UNSUPPORTED, the fallback signal of
    // every other string-valued root a host may hand in (it keeps its Go evaluator); a numeric root declared TSQ_BYTES is malformed.
    if (is_str[0] && p.result_type != TSQ_BYTES) { *why = "a string-valued root: declare result_type TSQ_BYTES and evaluate it with tsq_expr_eval_str"; return TSQ_ERR_UNSUPPORTED; }
    if (!is_str[0] && p.result_type == TSQ_BYTES) { *why = "result_type TSQ_BYTES needs a string-valued root"; return TSQ_ERR_INVALID; }
    if (p.result_type != TSQ_I64 && p.result_type != TSQ_F64 && p.result_type != TSQ_BYTES) { *why = "result_type must be TSQ_I64, TSQ_F64 or TSQ_BYTES"; return TSQ_ERR_INVALID; }
    return TSQ_OK;
}

#endif  // TSQ_DEVICE_H
