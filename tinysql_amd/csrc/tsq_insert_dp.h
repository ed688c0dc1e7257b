// tsq_insert_dp.h — the scalar core of INSERT ... SELECT's per-row step (tsq_insert.hip): one cell of the select's chunk -> the cell
// table.CastValue stores (table/column.go:142-189 over Datum.ConvertTo, types/datum.go:491-697), the NOT NULL decision of
// Column.HandleBadNull (table/column.go:290-299), and the operator of the auto-increment scan (adjustAutoIncrementDatum,
// executor/insert_common.go:594-638).  TSQ_HD and free of runtime calls so that the CPU test-suite compiles the very same code on
// the host (tests/insert_dp_main.cpp) against the Python restatement (tests/cast_ref.py) that is pinned on the reference's vectors.
//
// Every floating step below is ONE IEEE operation (the library is built with -ffp-contract=off, the host program too): f * shift,
// RoundFloat's f + copysign(0.5, f) and trunc, / shift — what Go's compiler emits for types.Round (types/helper.go:40-47).
#ifndef TSQ_INSERT_DP_H
#define TSQ_INSERT_DP_H

#include "tsq_device.h"
#include "tsq_rowenc_dp.h"  // the rune walk (utf8.DecodeRune)

// kind of the target column, derived from tsq_cast_col.tp / flags at create
#define TSQ_INS_SINT 0   // Tiny .. Longlong, signed        -> a TSQ_I64 column
#define TSQ_INS_UINT 1   // Tiny .. Longlong, UNSIGNED      -> a TSQ_U64 column
#define TSQ_INS_REAL 2   // Float -> a TSQ_F32 column, Double -> a TSQ_F64 column
#define TSQ_INS_STR 3    // Blob family, String, Varchar, VarString -> a TSQ_BYTES column

// what one cell reports (bits, or'ed)
#define TSQ_INS_EV_ERR 1u       // ConvertTo returned an error: it goes through sc.HandleTruncate (column.go:146-154), whatever its kind
#define TSQ_INS_EV_OVF_WARN 2u  // sc.HandleOverflow turned TruncateFloat's overflow into a warning (datum.go:558)
#define TSQ_INS_EV_NAN 4u       // a NaN reaching an integer target: Go's int64(NaN) is implementation defined -> TSQ_ERR_UNSUPPORTED
#define TSQ_INS_EV_TOO_LONG 8u  // types.ErrDataTooLong (datum.go:620-624)
#define TSQ_INS_EV_BAD_UTF8 16u // handleWrongUtf8Value (table/column.go:127-138)

// one table column as the kernels see it (built once by tsq_cast_create)
struct tsq_ins_col {
    int32_t src_col;    // index into the input columns, -1: the default
    int32_t src_type;   // TSQ_I64 / U64 / F32 / F64
    int32_t kind;       // TSQ_INS_*
    int32_t out_f32;    // TypeFloat: the result is narrowed to float32 (datum.go:544-545)
    uint32_t flags;     // TSQ_CAST_UNSIGNED | NOT_NULL | AUTO_INCREMENT | DEFAULT_NULL
    int32_t has_md;     // Flen and Decimal both given: TruncateFloat applies (datum.go:556)
    int64_t lo, hi;     // IntergerSignedLowerBound / UpperBound (types/convert.go:56-89)
    uint64_t ub;        // IntergerUnsignedUpperBound (types/convert.go:38-53)
    double shift, maxf; // math.Pow10(Decimal), GetMaxFloat(Flen, Decimal) (types/helper.go:63-68), computed on the host
    uint64_t def_bits;  // the default's 8 bytes (a float32 default: its 4 bytes)
    int32_t flen;       // a string target: FieldType.Flen, -1 = UnspecifiedLength
    int32_t is_char;    // a string target: TypeString (CHAR / BINARY)
    const uint8_t* def_bytes;  // a string target's default (the kernels get a device copy)
    int64_t def_len;
};

// ---- host only: tsq_cast_col -> tsq_ins_col, once per handle
// math.Pow10 as Go computes it (math/pow10.go): pow10postab32[n / 32] * pow10tab[n % 32], for a negative n pow10negtab32[-n / 32] /
// pow10tab[-n % 32]; the tables hold the correctly rounded literals, so Pow10(-2) is 1 / 1e2 and Pow10(40) is 1e32 * 1e8
inline double tsq_ins_pow10(int n) {
    static const double tab[32] = {1e0,  1e1,  1e2,  1e3,  1e4,  1e5,  1e6,  1e7,  1e8,  1e9,  1e10, 1e11, 1e12, 1e13, 1e14, 1e15,
                                   1e16, 1e17, 1e18, 1e19, 1e20, 1e21, 1e22, 1e23, 1e24, 1e25, 1e26, 1e27, 1e28, 1e29, 1e30, 1e31};
    static const double pos32[10] = {1e0, 1e32, 1e64, 1e96, 1e128, 1e160, 1e192, 1e224, 1e256, 1e288};
    static const double neg32[11] = {1e-0, 1e-32, 1e-64, 1e-96, 1e-128, 1e-160, 1e-192, 1e-224, 1e-256, 1e-288, 1e-320};
    if (0 <= n && n <= 308) return pos32[n / 32] * tab[n % 32];
    if (-323 <= n && n <= 0) return neg32[(-n) / 32] / tab[(-n) % 32];
    return n > 0 ? __builtin_inf() : 0.0;
}
// TSQ_OK, or TSQ_ERR_UNSUPPORTED (*why) for a column the Go path keeps, TSQ_ERR_INVALID for a malformed one
inline tsq_status tsq_ins_plan_col(const tsq_cast_col& s, tsq_ins_col* d, const char** why) {
    memset(d, 0, sizeof *d);
    *why = "";
    d->src_col = s.src_col;
    d->src_type = s.src_type;
    d->flags = s.flags;
    d->def_bits = s.def_bits;
    const bool is_int = s.tp == TSQ_TP_TINY || s.tp == TSQ_TP_SHORT || s.tp == TSQ_TP_INT24 || s.tp == TSQ_TP_LONG || s.tp == TSQ_TP_LONGLONG;
    const bool is_real = s.tp == TSQ_TP_FLOAT || s.tp == TSQ_TP_DOUBLE;
    const bool is_str = s.tp == TSQ_TP_VARCHAR || s.tp == TSQ_TP_VAR_STRING || s.tp == TSQ_TP_STRING || s.tp == TSQ_TP_TINY_BLOB || s.tp == TSQ_TP_MEDIUM_BLOB ||
                        s.tp == TSQ_TP_LONG_BLOB || s.tp == TSQ_TP_BLOB;
    if (s.tp == TSQ_TP_BIT) { *why = "a TypeBit target"; return TSQ_ERR_UNSUPPORTED; }
    if (!is_int && !is_real && !is_str) { *why = "unknown target type"; return TSQ_ERR_INVALID; }
    if (s.src_col >= 0) {
        if (s.src_type == TSQ_BYTES && is_real) { *why = "a string source into FLOAT / DOUBLE (StrToFloat)"; return TSQ_ERR_UNSUPPORTED; }
        if ((s.src_type == TSQ_F32 || s.src_type == TSQ_F64) && is_str) { *why = "a float source into a string target (strconv.FormatFloat)"; return TSQ_ERR_UNSUPPORTED; }
        if (s.src_type != TSQ_BYTES && s.src_type != TSQ_I64 && s.src_type != TSQ_U64 && s.src_type != TSQ_F32 && s.src_type != TSQ_F64) { *why = "unknown source type"; return TSQ_ERR_INVALID; }
    }
    if ((s.flags & TSQ_CAST_AUTO_INCREMENT) && (is_real || (s.flags & TSQ_CAST_UNSIGNED))) {
        *why = "an unsigned or floating auto-increment column";
        return TSQ_ERR_UNSUPPORTED;
    }
    if (is_str) {
        if (s.flags & TSQ_CAST_AUTO_INCREMENT) { *why = "a string auto-increment column"; return TSQ_ERR_INVALID; }
        if (s.def_len < 0 || (s.def_len > 0 && !s.def_bytes)) { *why = "bad default bytes"; return TSQ_ERR_INVALID; }
        d->kind = TSQ_INS_STR;
        d->flen = s.flen;
        d->is_char = s.tp == TSQ_TP_STRING ? 1 : 0;
        d->def_bytes = s.def_bytes;
        d->def_len = s.def_len;
        return TSQ_OK;
    }
    if (is_int) {
        d->kind = (s.flags & TSQ_CAST_UNSIGNED) ? TSQ_INS_UINT : TSQ_INS_SINT;
        const int bits = s.tp == TSQ_TP_TINY ? 8 : s.tp == TSQ_TP_SHORT ? 16 : s.tp == TSQ_TP_INT24 ? 24 : s.tp == TSQ_TP_LONG ? 32 : 64;
        d->hi = bits == 64 ? TSQ_I64MAX : ((int64_t)1 << (bits - 1)) - 1;
        d->lo = -d->hi - 1;
        d->ub = bits == 64 ? TSQ_U64MAX : ((uint64_t)1 << bits) - 1;
        return TSQ_OK;
    }
    d->kind = TSQ_INS_REAL;
    d->out_f32 = s.tp == TSQ_TP_FLOAT ? 1 : 0;
    d->has_md = (s.flen != -1 && s.decimal != -1) ? 1 : 0;
    if (d->has_md) {
        d->shift = tsq_ins_pow10(s.decimal);
        d->maxf = tsq_ins_pow10(s.flen - s.decimal) - tsq_ins_pow10(-s.decimal);
    }
    return TSQ_OK;
}
// the type of the output column of a planned column
inline int32_t tsq_ins_out_type(const tsq_ins_col& c) {
    return c.kind == TSQ_INS_STR ? TSQ_BYTES : c.kind == TSQ_INS_SINT ? TSQ_I64 : c.kind == TSQ_INS_UINT ? TSQ_U64 : c.out_f32 ? TSQ_F32 : TSQ_F64;
}

// types.RoundFloat (types/helper.go:28-34): half away from zero
TSQ_HD double tsq_ins_round_float(double f) {
    if (__builtin_fabs(f) < 0.5) return 0;
    return __builtin_trunc(f + __builtin_copysign(0.5, f));
}

// ConvertIntToInt / ConvertUintToInt / ConvertFloatToInt (types/convert.go:93-128) under toSignedInteger (datum.go:739-757)
TSQ_HD int64_t tsq_ins_int_to_int(int64_t v, int64_t lo, int64_t hi, uint32_t* ev) {
    if (v < lo) { *ev |= TSQ_INS_EV_ERR; return lo; }
    if (v > hi) { *ev |= TSQ_INS_EV_ERR; return hi; }
    return v;
}
TSQ_HD int64_t tsq_ins_uint_to_int(uint64_t v, int64_t hi, uint32_t* ev) {
    if (v > (uint64_t)hi) { *ev |= TSQ_INS_EV_ERR; return hi; }
    return (int64_t)v;
}
TSQ_HD int64_t tsq_ins_float_to_int(double f, int64_t lo, int64_t hi, uint32_t* ev) {
    if (f != f) { *ev |= TSQ_INS_EV_NAN; return 0; }
    const double val = tsq_ins_round_float(f);
    if (val < (double)lo) { *ev |= TSQ_INS_EV_ERR; return lo; }
    if (val >= (double)hi) {  // (float64(MaxInt64) is 2^63: the == case is what keeps 2^63 itself from wrapping)
        if (val != (double)hi) *ev |= TSQ_INS_EV_ERR;
        return hi;
    }
    return (int64_t)val;
}

// ConvertIntToUint / ConvertUintToUint / ConvertFloatToUint (types/convert.go:131-174) under convertToUint (datum.go:639-674);
// clip = sc.ShouldClipToZero() = InInsertStmt
TSQ_HD uint64_t tsq_ins_int_to_uint(int64_t v, uint64_t ub, bool clip, uint32_t* ev) {
    if (clip && v < 0) { *ev |= TSQ_INS_EV_ERR; return 0; }
    if ((uint64_t)v > ub) { *ev |= TSQ_INS_EV_ERR; return ub; }
    return (uint64_t)v;
}
TSQ_HD uint64_t tsq_ins_uint_to_uint(uint64_t v, uint64_t ub, uint32_t* ev) {
    if (v > ub) { *ev |= TSQ_INS_EV_ERR; return ub; }
    return v;
}
TSQ_HD uint64_t tsq_ins_float_to_uint(double f, uint64_t ub, bool clip, uint32_t* ev) {
    if (f != f) { *ev |= TSQ_INS_EV_NAN; return 0; }
    const double val = tsq_ins_round_float(f);
    if (val < 0) {
        *ev |= TSQ_INS_EV_ERR;
        if (clip) return 0;
        // uint64(int64(val)): below -2^63 Go's conversion is the amd64 instruction's "integer indefinite", 0x8000000000000000
        if (val < -9223372036854775808.0) return 0x8000000000000000ULL;
        return (uint64_t)(int64_t)val;
    }
    const double ubf = (double)ub;  // (float64(MaxUint64) is 2^64)
    if (val == ubf) return (uint64_t)TSQ_I64MAX;  // the reference answers MaxInt64 AT the bound of every unsigned type, without an error
    if (val > ubf) { *ev |= TSQ_INS_EV_ERR; return (uint64_t)TSQ_I64MAX; }
    return (uint64_t)val;
}

// TruncateFloat (types/helper.go:72-94) with types.Round inlined; *ovf: ErrOverflow "DOUBLE"
TSQ_HD double tsq_ins_truncate_float(double f, double shift, double maxf, bool* ovf) {
    *ovf = false;
    if (f != f) { *ovf = true; return 0; }
    if (!__builtin_isinf(f)) {
        const double tmp = f * shift;
        if (!__builtin_isinf(tmp)) f = tsq_ins_round_float(tmp) / shift;
    }
    if (f > maxf) { *ovf = true; return maxf; }
    if (f < -maxf) { *ovf = true; return -maxf; }
    return f;
}
// ProduceFloatWithSpecifiedTp (datum.go:553-566); overflow_as_warning = sc.OverflowAsWarning
TSQ_HD double tsq_ins_produce_float(double f, const tsq_ins_col& c, bool overflow_as_warning, uint32_t* ev) {
    if (c.has_md) {
        bool ovf;
        f = tsq_ins_truncate_float(f, c.shift, c.maxf, &ovf);
        if (ovf) {
            if (!overflow_as_warning) { *ev |= TSQ_INS_EV_ERR; return f; }  // (the unsigned test below is not reached)
            *ev |= TSQ_INS_EV_OVF_WARN;
        }
    }
    if ((c.flags & TSQ_CAST_UNSIGNED) && f < 0) { *ev |= TSQ_INS_EV_ERR; return 0; }
    return f;
}

TSQ_HD double tsq_ins_src_f64(int32_t src_type, uint64_t bits) {
    return src_type == TSQ_F32 ? (double)tsq_bits_f32((uint32_t)bits) : tsq_bits_f64(bits);
}

// Datum.ConvertTo for one NOT NULL fixed-width cell: `bits` = the source cell (a float32 source: its 4 bytes) -> the 8 bytes of
// the target cell (a TypeFloat target: its 4 bytes)
TSQ_HD uint64_t tsq_ins_cast_fixed(const tsq_ins_col& c, uint32_t stmt_flags, uint64_t bits, uint32_t* ev) {
    const bool clip = (stmt_flags & TSQ_CAST_IN_INSERT) != 0;
    if (c.kind == TSQ_INS_SINT) {
        if (c.src_type == TSQ_I64) return (uint64_t)tsq_ins_int_to_int((int64_t)bits, c.lo, c.hi, ev);
        if (c.src_type == TSQ_U64) return (uint64_t)tsq_ins_uint_to_int(bits, c.hi, ev);
        return (uint64_t)tsq_ins_float_to_int(tsq_ins_src_f64(c.src_type, bits), c.lo, c.hi, ev);
    }
    if (c.kind == TSQ_INS_UINT) {
        if (c.src_type == TSQ_I64) return tsq_ins_int_to_uint((int64_t)bits, c.ub, clip, ev);
        if (c.src_type == TSQ_U64) return tsq_ins_uint_to_uint(bits, c.ub, ev);
        return tsq_ins_float_to_uint(tsq_ins_src_f64(c.src_type, bits), c.ub, clip, ev);
    }
    double f;  // convertToFloat (datum.go:516-550)
    if (c.src_type == TSQ_I64) f = (double)(int64_t)bits;
    else if (c.src_type == TSQ_U64) f = (double)bits;
    else f = tsq_ins_src_f64(c.src_type, bits);
    f = tsq_ins_produce_float(f, c, (stmt_flags & TSQ_CAST_OVERFLOW_AS_WARNING) != 0, ev);
    if (c.out_f32) {
        const float g = (float)f;
        uint32_t u;
        memcpy(&u, &g, 4);
        return u;
    }
    return tsq_f64_bits(f);
}

// one cell of one table column, NULLs, defaults and the NOT NULL rule included.
//   in_null: the source cell is NULL (ignored for a column the statement did not name)
// Returns the cell's bits; *out_null.  *status: 0, or the TSQ_ERR_* the run fails with at this cell; *phase: 0 = the error belongs to
// getRow's cast loop (statement-column order), 1 = to fillRow's NOT NULL pass (table-column order), which runs after every cast of
// the row (insert_common.go:386-401, :455-469).  warn[0] += an overflow warning, warn[1] += a bad-null warning
TSQ_HD uint64_t tsq_ins_cell(const tsq_ins_col& c, uint32_t stmt_flags, uint64_t in_bits, bool in_null, bool* out_null, int32_t* status,
                             int32_t* phase, uint32_t* warn_overflow, uint32_t* warn_bad_null) {
    *status = 0;
    *phase = 0;
    *out_null = false;  // (also on the paths that return with a status: the caller builds bitmap words from it)
    uint64_t v = 0;
    bool isnull;
    if (c.src_col < 0) {  // fillColValue: the default (already cast by the host, once)
        isnull = (c.flags & TSQ_CAST_DEFAULT_NULL) != 0 || (c.flags & TSQ_CAST_AUTO_INCREMENT) != 0;
        v = isnull ? 0 : c.def_bits;
    } else if (in_null) {
        isnull = true;  // ConvertTo: NULL -> NULL
    } else {
        isnull = false;
        uint32_t ev = 0;
        v = tsq_ins_cast_fixed(c, stmt_flags, in_bits, &ev);
        if (ev & TSQ_INS_EV_NAN) {
            *status = TSQ_ERR_UNSUPPORTED;
            return 0;
        }
        if (ev & TSQ_INS_EV_OVF_WARN) *warn_overflow += 1;
        if ((ev & TSQ_INS_EV_ERR) && !(stmt_flags & TSQ_CAST_IGNORE_TRUNCATE)) {  // sc.HandleTruncate
            if (stmt_flags & TSQ_CAST_TRUNCATE_AS_WARNING) *warn_overflow += 1;
            else {
                *status = TSQ_ERR_OUT_OF_RANGE;
                return v;
            }
        }
    }
    // HandleBadNull; an auto-increment column gets its value from tsq_autoid_fill
    if (isnull && (c.flags & TSQ_CAST_NOT_NULL) && !(c.flags & TSQ_CAST_AUTO_INCREMENT)) {
        if (stmt_flags & TSQ_CAST_BAD_NULL_AS_WARNING) {
            *warn_bad_null += 1;
            isnull = false;
            v = 0;  // GetZeroValue: 0, 0.0
        } else {
            *status = TSQ_ERR_BAD_NULL;
            *phase = 1;
        }
    }
    *out_null = isnull;
    return v;
}

// ------------------------------------------------------------------ string targets
// strconv.FormatInt(v, 10) / FormatUint(v, 10) of a TSQ_I64 / TSQ_U64 cell: at most 20 ASCII bytes, kept in three words (byte i of the
// string = byte i % 8 of word i / 8) so that the kernels need no array; returns the length
TSQ_HD uint32_t tsq_ins_format_int(int32_t src_type, uint64_t bits, uint64_t* w0, uint64_t* w1, uint64_t* w2) {
    const bool neg = src_type == TSQ_I64 && (int64_t)bits < 0;
    uint64_t u = neg ? (uint64_t)0 - bits : bits;
    uint64_t lo = 0, mid = 0, hi = 0;
    uint32_t n = 0;
    do {  // every digit becomes the new first byte
        hi = (hi << 8) | (mid >> 56);
        mid = (mid << 8) | (lo >> 56);
        lo = (lo << 8) | (uint64_t)('0' + (u % 10u));
        u /= 10u;
        n++;
    } while (u);
    if (neg) {
        hi = (hi << 8) | (mid >> 56);
        mid = (mid << 8) | (lo >> 56);
        lo = (lo << 8) | (uint64_t)'-';
        n++;
    }
    *w0 = lo;
    *w1 = mid;
    *w2 = hi;
    return n;
}
TSQ_HD uint8_t tsq_ins_fmt_byte(uint64_t w0, uint64_t w1, uint64_t w2, uint32_t i) {
    const uint64_t w = i < 8u ? w0 : (i < 16u ? w1 : w2);
    return (uint8_t)(w >> (8u * (i & 7u)));
}
// tsq_ins_str_shape for a formatted integer: n ASCII bytes without a space — runes are bytes, nothing to trim, nothing invalid
TSQ_HD void tsq_ins_str_shape_ascii(const tsq_ins_col& c, uint64_t n, uint64_t* keep, uint64_t* pad, uint32_t* ev) {
    *keep = n;
    *pad = 0;
    if (c.flen < 0) return;
    const uint64_t fl = (uint64_t)c.flen;
    if (n > fl) { *ev |= TSQ_INS_EV_TOO_LONG; *keep = fl; }
    else if (c.is_char && (c.flags & TSQ_CAST_CHARSET_BIN) && n < fl && !(c.flags & (TSQ_CAST_CHARSET_UTF8 | TSQ_CAST_CHARSET_UTF8MB4))) *pad = fl - n;
}
// ProduceStrWithSpecifiedTp (types/datum.go:597-632) and what CastValue does to its result (table/column.go:155-188) for the string
// p[0 .. n): the cell is p[0 .. *keep) followed by *pad zero bytes.  Flen counts runes under utf8 / utf8mb4 (utf8.RuneCountInString: an
// invalid byte is a rune of width 1), bytes otherwise; BINARY(n) is padded; a non-binary CHAR loses its trailing spaces; the UTF-8
// walk cuts at the first invalid byte, or at the first 4-byte rune under 3-byte utf8 (a literal EF BF BD is valid).  Under strict
// truncation ErrDataTooLong is returned before the trim and the walk
TSQ_HD void tsq_ins_str_shape(const tsq_ins_col& c, uint32_t stmt_flags, const uint8_t* p, uint64_t n, uint64_t* keep, uint64_t* pad, uint32_t* ev) {
    const bool utf8cs = (c.flags & (TSQ_CAST_CHARSET_UTF8 | TSQ_CAST_CHARSET_UTF8MB4)) != 0, bin = (c.flags & TSQ_CAST_CHARSET_BIN) != 0;
    uint64_t k = n, pd = 0;
    if (c.flen >= 0) {
        const uint64_t fl = (uint64_t)c.flen;
        if (utf8cs) {
            if (n > fl) {  // (n bytes hold at most n runes)
                bool truncated, bad;
                const uint64_t pos = tsq_re_rune_prefix(p, n, fl, &truncated, &bad);
                if (truncated) { *ev |= TSQ_INS_EV_TOO_LONG; k = pos; }
            }
        } else if (n > fl) {
            *ev |= TSQ_INS_EV_TOO_LONG;
            k = fl;
        } else if (c.is_char && bin && n < fl) {
            pd = fl - n;
        }
    }
    *keep = k;
    *pad = pd;
    if ((*ev & TSQ_INS_EV_TOO_LONG) && !(stmt_flags & (TSQ_CAST_IGNORE_TRUNCATE | TSQ_CAST_TRUNCATE_AS_WARNING))) return;
    if (c.is_char && !bin)
        while (k > 0 && p[k - 1] == ' ') k--;  // truncateTrailingSpaces
    if (!(stmt_flags & TSQ_CAST_SKIP_UTF8_CHECK) && utf8cs) {
        uint64_t i = 0;
        while (i < k) {
            if (i + 8 <= k) {  // eight ASCII bytes at once (what most cells are made of): one load instead of eight
                uint64_t x;
                memcpy(&x, p + i, 8);
                if (!(x & 0x8080808080808080ULL)) { i += 8; continue; }
            }
            bool ok;
            const uint32_t w = tsq_re_rune_width(p + i, k - i, &ok);
            if (!ok || (w > 3u && (c.flags & TSQ_CAST_CHARSET_UTF8))) { *ev |= TSQ_INS_EV_BAD_UTF8; k = i; break; }
            i += w;
        }
    }
    *keep = k;
}
// one cell of a string column, NULLs, defaults and the NOT NULL rule included; p[0 .. n): the source string (an integer source:
// already formatted; a column the statement does not name: ignored).  The cell is src[0 .. *keep) + *pad zero bytes, src = p, or the
// default for an unnamed column (*from_default), or nothing.  warn: [0] overflow [1] bad null [2] data too long [3] bad utf8
TSQ_HD void tsq_ins_str_cell(const tsq_ins_col& c, uint32_t stmt_flags, const uint8_t* p, uint64_t n, bool in_null, uint64_t* keep, uint64_t* pad, bool* from_default,
                             bool* out_null, int32_t* status, int32_t* phase, uint32_t* warn) {
    *status = 0;
    *phase = 0;
    *keep = 0;
    *pad = 0;
    *from_default = false;
    *out_null = false;
    bool isnull;
    if (c.src_col < 0) {
        isnull = (c.flags & TSQ_CAST_DEFAULT_NULL) != 0;
        if (!isnull) { *from_default = true; *keep = (uint64_t)c.def_len; }  // (cast by the host, once)
    } else if (in_null) {
        isnull = true;
    } else {
        isnull = false;
        uint32_t ev = 0;
        if (c.src_type == TSQ_BYTES) tsq_ins_str_shape(c, stmt_flags, p, n, keep, pad, &ev);
        else tsq_ins_str_shape_ascii(c, n, keep, pad, &ev);  // (p is not read: the caller holds the digits in registers)
        if (!(stmt_flags & TSQ_CAST_IGNORE_TRUNCATE)) {  // sc.HandleTruncate, in ProduceStrWithSpecifiedTp and in CastValue
            const bool warn_only = (stmt_flags & TSQ_CAST_TRUNCATE_AS_WARNING) != 0;
            if (ev & TSQ_INS_EV_TOO_LONG) {
                if (warn_only) warn[2] += 1;
                else { *status = TSQ_ERR_DATA_TOO_LONG; return; }
            }
            if (ev & TSQ_INS_EV_BAD_UTF8) {
                if (warn_only) warn[3] += 1;
                else { *status = TSQ_ERR_BAD_UTF8; return; }
            }
        }
    }
    if (isnull && (c.flags & TSQ_CAST_NOT_NULL)) {
        if (stmt_flags & TSQ_CAST_BAD_NULL_AS_WARNING) {
            warn[1] += 1;
            isnull = false;  // GetZeroValue (table/column.go:373-382): BINARY(n) is n zero bytes, every other string type ""
            *keep = 0;
            *pad = (c.is_char && (c.flags & TSQ_CAST_CHARSET_BIN) && c.flen > 0) ? (uint64_t)c.flen : 0;
        } else {
            *status = TSQ_ERR_BAD_NULL;
            *phase = 1;
        }
    }
    *out_null = isnull;
}

// one cell of an INTEGER column fed by a string: toSignedInteger's / convertToUint's string arms (types/datum.go:751-757, :654-663) over
// types.StrToInt / StrToUint (tsq_str_to_int / tsq_str_to_uint with the statement's TSQ_STRCTX_* flags), NULLs and the NOT NULL rule included.
//   signed:   the parsed value is clipped to the type (ConvertIntToInt) and ALWAYS stored; the parse's error wins over the clip's
//   unsigned: the parse's ErrOverflow returns at once unless sc.ShouldIgnoreOverflowError() (InInsertStmt && TruncateAsWarning); then
//             ConvertUintToUint, whose error returns at once too; only then the parse's error (overflow or truncation) goes with the value.
//             Both early returns hand back the ZERO Datum — a NULL: when sc.HandleTruncate swallows the error the cell is NULL
// warn: [0] overflow, [1] bad null, [2] truncated (ErrTruncatedWrongVal: appended by StrToInt itself, or the returned error as a warning)
TSQ_HD uint64_t tsq_ins_cell_str_int(const tsq_ins_col& c, uint32_t stmt_flags, uint32_t str_ctx, const uint8_t* p, uint32_t n, bool in_null, bool* out_null,
                                     int32_t* status, int32_t* phase, uint32_t* warn) {
    *status = 0;
    *phase = 0;
    *out_null = false;
    uint64_t v = 0;
    bool isnull = in_null;
    if (!in_null) {
        uint32_t f, ev = 0;
        int err = 0;  // 1: ErrOverflow, 2: ErrTruncatedWrongVal
        bool null_out = false;
        if (c.kind == TSQ_INS_SINT) {
            int64_t x = 0;
            f = tsq_str_to_int(p, n, str_ctx, &x);
            v = (uint64_t)tsq_ins_int_to_int(x, c.lo, c.hi, &ev);
            err = (f & TSQ_S2I_ERR_OVF) ? 1 : (f & TSQ_S2I_ERR_TRUNC) ? 2 : (ev ? 1 : 0);
        } else {
            uint64_t x = 0;
            f = tsq_str_to_uint(p, n, str_ctx, &x);
            const bool ignore_ovf = (stmt_flags & TSQ_CAST_IN_INSERT) && (stmt_flags & TSQ_CAST_TRUNCATE_AS_WARNING);
            if ((f & TSQ_S2I_ERR_OVF) && !ignore_ovf) {
                err = 1;
                null_out = true;
            } else {
                v = tsq_ins_uint_to_uint(x, c.ub, &ev);
                if (ev) {
                    err = 1;
                    null_out = true;
                } else {
                    err = (f & TSQ_S2I_ERR_OVF) ? 1 : (f & TSQ_S2I_ERR_TRUNC) ? 2 : 0;
                }
            }
        }
        if (f & TSQ_S2I_TRUNC_WARN) warn[2] += 1;
        if (f & TSQ_S2I_OVF_WARN) warn[0] += 1;
        if (err && !(stmt_flags & TSQ_CAST_IGNORE_TRUNCATE)) {  // sc.HandleTruncate (table/column.go:146-154)
            if (stmt_flags & TSQ_CAST_TRUNCATE_AS_WARNING) warn[err == 1 ? 0 : 2] += 1;
            else {
                *status = err == 1 ? TSQ_ERR_OUT_OF_RANGE : TSQ_ERR_TRUNCATED_WRONG_VALUE;
                return v;
            }
        }
        if (null_out) {
            isnull = true;
            v = 0;
        }
    }
    if (isnull && (c.flags & TSQ_CAST_NOT_NULL) && !(c.flags & TSQ_CAST_AUTO_INCREMENT)) {
        if (stmt_flags & TSQ_CAST_BAD_NULL_AS_WARNING) {
            warn[1] += 1;
            isnull = false;
            v = 0;
        } else {
            *status = TSQ_ERR_BAD_NULL;
            *phase = 1;
        }
    }
    *out_null = isnull;
    return v;
}

// the position of a failing cell as one word: the smallest word of a run is the error the reference stops at
//   row | phase | order (statement column of a cast, table column of a NOT NULL failure) | table column | status
#define TSQ_INS_ERR_NONE 0xffffffffffffffffULL
TSQ_HD uint64_t tsq_ins_errword(int64_t row, int32_t phase, int32_t order, int32_t table_col, int32_t status) {
    return ((uint64_t)row << 19) | ((uint64_t)(phase & 1) << 18) | ((uint64_t)(order & 31) << 13) | ((uint64_t)(table_col & 31) << 8) | (uint64_t)(status & 255);
}
TSQ_HD int64_t tsq_ins_err_row(uint64_t w) { return (int64_t)(w >> 19); }
TSQ_HD int32_t tsq_ins_err_col(uint64_t w) { return (int32_t)((w >> 8) & 31); }
TSQ_HD int32_t tsq_ins_err_status(uint64_t w) { return (int32_t)(w & 255); }

// ------------------------------------------------------------------ auto ids
// adjustAutoIncrementDatum over one allocator with increment 1: the allocator's state s after a row is f(s before) with
// f(x) = max(x + a, b): an explicit id v is (a, b) = (0, v) (RebaseAutoID), an allocation is (1, -inf), a row that leaves the
// allocator alone (a 0 under NO_AUTO_VALUE_ON_ZERO) is (0, -inf).  Functions of this form compose to one of the same form, so the
// ids of a chunk are a scan.  -inf is INT64_MIN (max(x, INT64_MIN) = x, and it is kept by every addition); a sum that leaves int64
// saturates at INT64_MAX and sets `ovf` for good: the allocator would have passed INT64_MAX inside the stretch the element stands for.
#define TSQ_AID_NEG_INF ((int64_t)0x8000000000000000LL)
struct tsq_aid_op {
    int64_t a, b;
    int32_t ovf;
};
TSQ_HD tsq_aid_op tsq_aid_identity() { return tsq_aid_op{0, TSQ_AID_NEG_INF, 0}; }
TSQ_HD int64_t tsq_aid_add(int64_t b, int64_t a, int32_t* ovf) {  // a >= 0
    if (b == TSQ_AID_NEG_INF) return b;
    int64_t r;
    if (__builtin_add_overflow(b, a, &r)) { *ovf = 1; return TSQ_I64MAX; }
    return r;
}
// first f, then g
TSQ_HD tsq_aid_op tsq_aid_compose(const tsq_aid_op& f, const tsq_aid_op& g) {
    tsq_aid_op r;
    r.ovf = f.ovf | g.ovf;
    int64_t a;
    if (__builtin_add_overflow(f.a, g.a, &a)) { r.ovf = 1; a = TSQ_I64MAX; }
    r.a = a;
    const int64_t fb = tsq_aid_add(f.b, g.a, &r.ovf);
    r.b = fb > g.b ? fb : g.b;
    return r;
}
TSQ_HD int64_t tsq_aid_apply(const tsq_aid_op& f, int64_t x, int32_t* ovf) {
    *ovf |= f.ovf;
    int64_t r;
    if (__builtin_add_overflow(x, f.a, &r)) { *ovf = 1; r = TSQ_I64MAX; }
    return r > f.b ? r : f.b;
}
// row kinds
#define TSQ_AID_EXPLICIT 0
#define TSQ_AID_ALLOC 1
#define TSQ_AID_KEEP 2
TSQ_HD int tsq_aid_row_kind(int64_t v, bool isnull, uint32_t flags) {
    if (!isnull && v != 0) return TSQ_AID_EXPLICIT;
    if (isnull || !(flags & TSQ_AUTOID_NO_AUTO_VALUE_ON_ZERO)) return TSQ_AID_ALLOC;
    return TSQ_AID_KEEP;
}
TSQ_HD tsq_aid_op tsq_aid_row_op(int kind, int64_t v) {
    if (kind == TSQ_AID_EXPLICIT) return tsq_aid_op{0, v, 0};
    if (kind == TSQ_AID_ALLOC) return tsq_aid_op{1, TSQ_AID_NEG_INF, 0};
    return tsq_aid_identity();
}

#endif
