// tsq_rowenc.hip — the write path of the storage side on the GPU: chunk rows -> stored row values (row format v2) and chunk rows ->
// index entries.
//
// Replaces the per-row loops of the reference's writers: rowcodec.Encoder.Encode (util/rowcodec/encoder.go:34-194) as tables.AddRecord
// reaches it through tablecodec.EncodeRow (tablecodec/tablecodec.go:129) — the inverse of tsq_rowcodec_decode — and index.GenIndexKey
// (table/tables/index.go:161-189) + the value index.Create stores (:224-244) as the ADD INDEX backfill runs them per row
// (ddl/index.go:742-921) — the inverse of tsq_indexkeys_decode.  Rows are independent, their bytes are packed back to back, so the byte
// position of a row is a prefix sum: the three-kernel shape of tsq_encode.hip (K16a-c).
//   K19a k_renc_size / k_ienc_size : every workgroup owns a contiguous range of 256-row tiles and adds up the bytes of its rows
//   K19b k_wenc_scan               : <= 1024 workgroup totals -> the byte position where each workgroup starts
//   K19c k_renc_emit / k_ienc_emit : per tile: row lengths again, block-wide exclusive scan -> row positions (handed to the caller), every
//                                    lane writes its row into an LDS image of the tile, the workgroup copies the image to its place in the
//                                    output with aligned 16-byte stores (tsq_enc_copy_plan).  A tile that does not fit the image is
//                                    written to its place directly.  A var-len cell of wave_copy_min bytes or more is copied by the whole
//                                    wave (consecutive lanes, consecutive bytes) instead of its row's lane.
// The lane that owns a row does what is specific to the stored-row format: one walk over the columns in id order (the order is the
// same for every row: one permutation computed on the host) that puts a not-null column's id, value and end offset and a null column's
// id behind the not-null ones; the `large` decision; u8 / u32 ids and u16 / u32 offsets.
// HBM-bound byte work, no MFMA.  Algorithmic bytes per row: the columns read twice (8 B per fixed-width cell, offsets + bytes of a
// var-len cell; the size pass does not read the bytes of a plain string cell) + the bytes written (+ 8 B row offset).
#include "tsq_internal.h"
#include "tsq_radix.h"
#include "tsq_encode_dp.h"
#include "tsq_rowenc_dp.h"

#define WENC_NT 256
#define WENC_MAXWG 1024
#define WENC_WAVE_COPY_DEFAULT 64  // bytes; profiles/write_path_ab.txt

struct WencCols {
    const void* data[TSQ_MAX_COLS];
    const uint8_t* nulls[TSQ_MAX_COLS];  // nullptr: no NULLs
    const int64_t* offs[TSQ_MAX_COLS];   // var-len columns: offsets[nrows + 1] into data
    int32_t type[TSQ_MAX_COLS];
    int32_t n_cols;
};
struct WencShape {  // the launch: workgroup b owns tiles [b * tiles_per_wg, (b + 1) * tiles_per_wg)
    int64_t nrows, n_tiles, tiles_per_wg;
    int32_t n_wg;
    uint32_t lds_bytes;      // LDS image of the launch: a tile that does not fit is written to the output directly
    uint32_t wave_copy_min;  // var-len cells of at least this many bytes are copied by the wave
    uint32_t* err;           // [2] error words of the size pass
    unsigned long long* wg_bytes;  // [n_sums][n_wg + 1]: totals (size pass), then exclusive starts + grand total (scan)
};
struct RencArgs {
    WencCols c;
    WencShape s;
    uint32_t ids[TSQ_MAX_COLS];   // the column ids
    uint8_t perm[TSQ_MAX_COLS];   // the columns in id order
    uint32_t bit_mask;            // bit c: a TSQ_RC_BIT column
    uint32_t id_large;            // a column id exceeds 255
    uint8_t* out;
    int64_t* row_offsets;         // nullptr or [nrows + 1]
};
struct IencArgs {
    WencCols c;
    WencShape s;
    int32_t prefix_len[TSQ_MAX_COLS];  // -1 = whole cell
    uint32_t utf8_mask;                // bit c: prefix_len[c] counts runes
    uint32_t unique;
    uint64_t table_u, index_u;         // EncodeIntToCmpUint of the two ids
    const int64_t* handles;
    uint8_t* keys;
    int64_t* key_offsets;    // [nrows + 1]
    uint8_t* values;
    int64_t* value_offsets;  // [nrows + 1]
    uint8_t* distinct;       // nullptr or [nrows]
};

#define WENC_ERR_BIT_CELL 0   // err[0]: a bit column's cell is not 1..8 bytes long
#define WENC_ERR_TOO_LONG 1   // err[1]: a row's value bytes reach 2^32 | an invalid byte inside the kept rune prefix of a truncated cell

namespace {

__device__ __forceinline__ bool wenc_notnull(const WencCols& c, int k, int64_t r) {
    const uint8_t* bm = c.nulls[k];
    return bm ? ((bm[r >> 3] >> (r & 7)) & 1) != 0 : true;
}
// the 8 bytes a fixed-width column stores for row r as the encoders want them (a float32 widened to its double image)
__device__ __forceinline__ uint64_t wenc_load(const WencCols& c, int k, int64_t r) {
    if (c.type[k] == TSQ_F32) return tsq_f64_bits((double)((const float*)c.data[k])[r]);
    return ((const uint64_t*)c.data[k])[r];
}

// 64-bit block-wide exclusive scan (a tile of 256 stored rows may pass 4 GiB); s_wsum: NT / 64 words
template <int NT>
__device__ __forceinline__ uint64_t block_excl_scan64(uint64_t v, unsigned long long* s_wsum, uint64_t* total) {
    const uint32_t lane = threadIdx.x & 63u;
    unsigned long long inc = v;
#pragma unroll
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(inc, o, 64);
        if (lane >= (uint32_t)o) inc += y;
    }
    const int w = threadIdx.x >> 6;
    if (lane == 63u) s_wsum[w] = inc;
    __syncthreads();
    uint64_t pre = 0, tot = 0;
#pragma unroll
    for (int i = 0; i < NT / 64; i++) {
        const uint64_t x = s_wsum[i];
        pre += i < w ? x : 0u;
        tot += x;
    }
    *total = tot;
    return pre + (inc - v);
}

// workgroup sum of `sum` -> dst[blockIdx.x]
__device__ __forceinline__ void wenc_block_sum(unsigned long long sum, unsigned long long* s_sum, unsigned long long* dst) {
    const uint32_t tid = threadIdx.x;
    for (int o = 32; o > 0; o >>= 1) sum += __shfl_xor(sum, o, 64);
    if ((tid & 63u) == 0) s_sum[tid >> 6] = sum;
    __syncthreads();
    if (tid == 0) {
        unsigned long long tot = 0;
        for (int w = 0; w < WENC_NT / 64; w++) tot += s_sum[w];
        dst[blockIdx.x] = tot;
    }
    __syncthreads();
}

// n_sums arrays of <= 1024 workgroup totals: one thread each turns them into exclusive starts; [n_wg] = the grand total
__global__ void k_wenc_scan(WencShape s, int n_sums) {
    if (blockIdx.x == 0 && (int)threadIdx.x < n_sums) {
        unsigned long long* w = s.wg_bytes + (size_t)threadIdx.x * ((size_t)s.n_wg + 1);
        unsigned long long run = 0;
        for (int b = 0; b < s.n_wg; b++) {
            const unsigned long long v = w[b];
            w[b] = run;
            run += v;
        }
        w[s.n_wg] = run;
    }
}

// the staged tile leaves LDS: whole 16-byte vectors aligned, the bytes shared with a neighbouring tile's vector one by one
__device__ __forceinline__ void wenc_copy_out(uint8_t* out, int64_t base, const tsq_enc_copy& plan, const uint4* s_img) {
    const uint32_t tid = threadIdx.x;
    const uint8_t* img = (const uint8_t*)s_img;
    uint8_t* g = out + base - plan.skew;  // 16-byte aligned by construction
    if (tid < 16 && plan.skew + tid < plan.head_end) g[plan.skew + tid] = img[plan.skew + tid];
    if (tid >= 16 && tid < 32 && plan.tail_lo + (tid - 16) < plan.tail_end) g[plan.tail_lo + (tid - 16)] = img[plan.tail_lo + (tid - 16)];
    for (uint32_t i = plan.body_lo + tid; i < plan.body_hi; i += WENC_NT) ((uint4*)g)[i] = s_img[i];
}

// ---------------------------------------------------------------------------------------------------------------- stored rows
struct RencRow {
    uint32_t n_notnull;
    uint32_t err;      // bit 0: bit cell of a bad length, bit 1: value bytes reach 2^32
    uint64_t value_bytes;
    bool large;
    uint64_t len;
};
__device__ __forceinline__ RencRow renc_row(const RencArgs& a, int64_t r) {
    RencRow w;
    w.n_notnull = 0;
    w.err = 0;
    w.value_bytes = 0;
    for (int k = 0; k < a.c.n_cols; k++) {
        if (!wenc_notnull(a.c, k, r)) continue;
        w.n_notnull++;
        if (a.c.type[k] == TSQ_BYTES) {
            const int64_t s0 = a.c.offs[k][r];
            const uint64_t n = (uint64_t)(a.c.offs[k][r + 1] - s0);
            if ((a.bit_mask >> k) & 1u) {
                uint64_t v;
                if (!tsq_re_bit_value((const uint8_t*)a.c.data[k] + s0, n <= 8 ? n : 0, &v)) w.err |= 1u;
                w.value_bytes += tsq_re_uint_width(v);
            } else {
                w.value_bytes += n;
            }
            continue;
        }
        uint64_t le;
        w.value_bytes += tsq_re_value(a.c.type[k], wenc_load(a.c, k, r), &le);
    }
    if (w.value_bytes >> 32) w.err |= 2u;
    w.large = tsq_re_large(a.id_large != 0, w.value_bytes);
    w.len = tsq_re_row_len(w.large, w.n_notnull, (uint32_t)a.c.n_cols - w.n_notnull, w.value_bytes);
    return w;
}

__global__ void __launch_bounds__(WENC_NT) k_renc_size(RencArgs a) {
    __shared__ unsigned long long s_sum[WENC_NT / 64];
    const uint32_t tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * a.s.tiles_per_wg, t1 = t0 + a.s.tiles_per_wg < a.s.n_tiles ? t0 + a.s.tiles_per_wg : a.s.n_tiles;
    unsigned long long sum = 0;
    uint32_t err = 0;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t r = t * WENC_NT + tid;
        if (r < a.s.nrows) {
            const RencRow w = renc_row(a, r);
            sum += w.len;
            err |= w.err;
        }
    }
    if (err & 1u) a.s.err[WENC_ERR_BIT_CELL] = 1u;
    if (err & 2u) a.s.err[WENC_ERR_TOO_LONG] = 1u;
    wenc_block_sum(sum, s_sum, a.s.wg_bytes);
}

__device__ __forceinline__ void wenc_put(uint8_t* d, uint64_t le, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) d[i] = (uint8_t)(le >> (8 * i));
}

__global__ void __launch_bounds__(WENC_NT) k_renc_emit(RencArgs a) {
    extern __shared__ uint4 s_img[];  // the tile's bytes at [skew, skew + T)
    __shared__ unsigned long long s_wsum[WENC_NT / 64];
    uint8_t* img = (uint8_t*)s_img;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int64_t t0 = (int64_t)blockIdx.x * a.s.tiles_per_wg, t1 = t0 + a.s.tiles_per_wg < a.s.n_tiles ? t0 + a.s.tiles_per_wg : a.s.n_tiles;
    int64_t base = (int64_t)a.s.wg_bytes[blockIdx.x];
    const int n_cols = a.c.n_cols;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t r = t * WENC_NT + tid;
        const bool live = r < a.s.nrows;
        RencRow w;
        w.len = 0;
        w.n_notnull = 0;
        w.large = false;
        if (live) w = renc_row(a, r);
        uint64_t T;
        const uint64_t ex = block_excl_scan64<WENC_NT>(w.len, s_wsum, &T);
        // a tile whose bytes do not fit the LDS image (rows with long strings) is written to its place directly, row by row
        const uint32_t skew = (uint32_t)(((uint64_t)(uintptr_t)a.out + (uint64_t)base) & 15u);
        const bool staged = (uint64_t)skew + T + 16 <= (uint64_t)a.s.lds_bytes;  // workgroup uniform
        const tsq_enc_copy plan = tsq_enc_copy_plan((uint64_t)(uintptr_t)a.out, base, staged ? (uint32_t)T : 0u);
        uint8_t* dst = staged ? img + skew + ex : a.out + base + ex;
        const uint32_t idw = w.large ? 4u : 1u, ow = w.large ? 4u : 2u;
        const uint64_t offs_at = 6u + (uint64_t)n_cols * idw, data_at = offs_at + (uint64_t)w.n_notnull * ow;
        if (live) {
            if (a.row_offsets) a.row_offsets[r] = base + (int64_t)ex;
            wenc_put(dst, tsq_re_header(w.large, w.n_notnull, (uint32_t)n_cols - w.n_notnull), 6);
        }
        uint32_t i_nn = 0, i_null = 0;
        uint64_t run = 0;  // value bytes so far
        for (int q = 0; q < n_cols; q++) {  // the columns in id order: every lane of the workgroup walks them together
            const int k = a.perm[q];
            const bool is_str = a.c.type[k] == TSQ_BYTES && !((a.bit_mask >> k) & 1u);  // uniform
            const bool nn = live && wenc_notnull(a.c, k, r);
            if (live && !nn) {  // a null column: its id behind the not-null ids
                wenc_put(dst + 6u + (uint64_t)(w.n_notnull + i_null) * idw, a.ids[k], idw);
                i_null++;
            }
            if (nn) wenc_put(dst + 6u + (uint64_t)i_nn * idw, a.ids[k], idw);
            if (!is_str) {
                if (nn) {
                    uint64_t le;
                    uint32_t n;
                    if (a.c.type[k] == TSQ_BYTES) {  // a bit column: the unsigned integer its bytes spell
                        const int64_t s0 = a.c.offs[k][r];
                        const uint64_t cn = (uint64_t)(a.c.offs[k][r + 1] - s0);
                        tsq_re_bit_value((const uint8_t*)a.c.data[k] + s0, cn <= 8 ? cn : 0, &le);
                        n = tsq_re_uint_width(le);
                    } else {
                        n = tsq_re_value(a.c.type[k], wenc_load(a.c, k, r), &le);
                    }
                    wenc_put(dst + data_at + run, le, n);
                    run += n;
                }
            } else {
                int64_t s0 = 0;
                uint64_t n = 0;
                if (nn) {
                    s0 = a.c.offs[k][r];
                    n = (uint64_t)(a.c.offs[k][r + 1] - s0);
                }
                const uint8_t* col = (const uint8_t*)a.c.data[k];
                const bool by_wave = nn && n >= (uint64_t)a.s.wave_copy_min;
                if (nn && !by_wave) {
                    uint8_t* d = dst + data_at + run;
                    for (uint64_t i = 0; i < n; i++) d[i] = col[s0 + i];
                }
                // long cells: one after the other, each copied by the 64 lanes of its row's wave
                unsigned long long m = __ballot(by_wave);
                const uint64_t my_at = (staged ? (uint64_t)skew : (uint64_t)base) + ex + data_at + run;  // into img | into out
                while (m) {
                    const int l = __ffsll(m) - 1;
                    m &= m - 1;
                    const uint64_t at = __shfl((unsigned long long)my_at, l, 64), cn = __shfl((unsigned long long)n, l, 64);
                    const int64_t cs = (int64_t)__shfl((unsigned long long)s0, l, 64);
                    const uint8_t* src = col + cs;
                    if (staged) {
                        uint8_t* d = img + at;
                        for (uint64_t i = lane; i < cn; i += 64) d[i] = src[i];
                    } else {
                        uint8_t* d = a.out + at;
                        const uint64_t nv = cn >> 3;  // eight bytes per lane (global loads and stores take any byte address), then the tail
                        for (uint64_t i = lane; i < nv; i += 64) {
                            uint64_t x;
                            memcpy(&x, src + 8 * i, 8);
                            memcpy(d + 8 * i, &x, 8);
                        }
                        for (uint64_t i = (nv << 3) + lane; i < cn; i += 64) d[i] = src[i];
                    }
                }
                run += n;
            }
            if (nn) {
                wenc_put(dst + offs_at + (uint64_t)i_nn * ow, run, ow);
                i_nn++;
            }
        }
        __syncthreads();
        if (staged) wenc_copy_out(a.out, base, plan, s_img);
        __syncthreads();  // the image (and s_wsum) are reused by the next tile
        base += (int64_t)T;
    }
    if (tid == 0 && a.row_offsets && t1 == a.s.n_tiles && t1 > t0) a.row_offsets[a.s.nrows] = base;  // the workgroup that owns the last tile
}

// ---------------------------------------------------------------------------------------------------------------- index entries
struct IencRow {
    uint64_t len;   // key bytes
    uint32_t vlen;  // value bytes: 8 (the handle) or 1 ('0')
    bool distinct, bad;
};
// bytes of column k's cell the key holds (TruncateIndexValuesIfNeeded)
__device__ __forceinline__ uint64_t ienc_cell_len(const IencArgs& a, int k, int64_t s0, uint64_t n, bool* bad) {
    return tsq_re_index_cell_len((const uint8_t*)a.c.data[k] + s0, n, a.prefix_len[k], (a.utf8_mask >> k) & 1u, bad);
}
__device__ __forceinline__ IencRow ienc_row(const IencArgs& a, int64_t r) {
    IencRow w;
    w.len = 19u;
    w.bad = false;
    bool any_null = false;
    for (int k = 0; k < a.c.n_cols; k++) {
        const bool nn = wenc_notnull(a.c, k, r);
        any_null = any_null || !nn;
        if (!nn) { w.len += 1u; continue; }  // NilFlag
        if (a.c.type[k] == TSQ_BYTES) {
            const int64_t s0 = a.c.offs[k][r];
            bool bad;
            w.len += tsq_enc_membytes_len(ienc_cell_len(a, k, s0, (uint64_t)(a.c.offs[k][r + 1] - s0), &bad));
            w.bad = w.bad || bad;
        } else {
            w.len += 9u;
        }
    }
    w.distinct = a.unique && !any_null;
    if (!w.distinct) w.len += 9u;  // the handle as an int datum
    w.vlen = w.distinct ? 8u : 1u;
    return w;
}

__global__ void __launch_bounds__(WENC_NT) k_ienc_size(IencArgs a) {
    __shared__ unsigned long long s_sum[WENC_NT / 64];
    const uint32_t tid = threadIdx.x;
    const int64_t t0 = (int64_t)blockIdx.x * a.s.tiles_per_wg, t1 = t0 + a.s.tiles_per_wg < a.s.n_tiles ? t0 + a.s.tiles_per_wg : a.s.n_tiles;
    unsigned long long sum = 0, vsum = 0;
    bool bad = false;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t r = t * WENC_NT + tid;
        if (r < a.s.nrows) {
            const IencRow w = ienc_row(a, r);
            sum += w.len;
            vsum += w.vlen;
            bad = bad || w.bad;
        }
    }
    if (bad) a.s.err[WENC_ERR_TOO_LONG] = 1u;
    wenc_block_sum(sum, s_sum, a.s.wg_bytes);
    wenc_block_sum(vsum, s_sum, a.s.wg_bytes + a.s.n_wg + 1);
}

__device__ __forceinline__ void wenc_put_datum(uint8_t* d, uint64_t lo, uint32_t hi, uint32_t n) {
    for (uint32_t i = 0; i < n; i++) d[i] = (uint8_t)(i < 8 ? lo >> (8 * i) : hi >> (8 * (i - 8)));
}

__global__ void __launch_bounds__(WENC_NT) k_ienc_emit(IencArgs a) {
    extern __shared__ uint4 s_img[];
    __shared__ unsigned long long s_wsum[WENC_NT / 64];
    uint8_t* img = (uint8_t*)s_img;
    const uint32_t tid = threadIdx.x, lane = tid & 63u;
    const int64_t t0 = (int64_t)blockIdx.x * a.s.tiles_per_wg, t1 = t0 + a.s.tiles_per_wg < a.s.n_tiles ? t0 + a.s.tiles_per_wg : a.s.n_tiles;
    int64_t base = (int64_t)a.s.wg_bytes[blockIdx.x], vbase = (int64_t)a.s.wg_bytes[a.s.n_wg + 1 + blockIdx.x];
    const int n_cols = a.c.n_cols;
    for (int64_t t = t0; t < t1; t++) {
        const int64_t r = t * WENC_NT + tid;
        const bool live = r < a.s.nrows;
        IencRow w;
        w.len = 0;
        w.vlen = 0;
        w.distinct = false;
        if (live) w = ienc_row(a, r);
        // one scan for both: the value bytes of a tile (<= 2048) ride in the top 16 bits
        uint64_t TT;
        const uint64_t exx = block_excl_scan64<WENC_NT>(w.len | ((uint64_t)w.vlen << 48), s_wsum, &TT);
        const uint64_t T = TT & 0xffffffffffffULL, ex = exx & 0xffffffffffffULL, vT = TT >> 48, vex = exx >> 48;
        const uint32_t skew = (uint32_t)(((uint64_t)(uintptr_t)a.keys + (uint64_t)base) & 15u);
        const bool staged = (uint64_t)skew + T + 16 <= (uint64_t)a.s.lds_bytes;  // workgroup uniform
        const tsq_enc_copy plan = tsq_enc_copy_plan((uint64_t)(uintptr_t)a.keys, base, staged ? (uint32_t)T : 0u);
        uint8_t* dst = staged ? img + skew + ex : a.keys + base + ex;
        uint64_t pos = 0;
        int64_t handle = 0;
        if (live) {
            handle = a.handles[r];
            a.key_offsets[r] = base + (int64_t)ex;
            a.value_offsets[r] = vbase + (int64_t)vex;
            if (a.distinct) a.distinct[r] = w.distinct ? 1 : 0;
            uint8_t* v = a.values + vbase + vex;
            if (w.distinct) {  // EncodeHandle: 8 bytes big endian
                for (int i = 0; i < 8; i++) v[i] = (uint8_t)((uint64_t)handle >> (56 - 8 * i));
            } else {
                v[0] = (uint8_t)'0';
            }
            // 't' | EncodeInt(table_id) | "_i" | EncodeInt(index_id)
            dst[0] = (uint8_t)'t';
            for (int i = 0; i < 8; i++) dst[1 + i] = (uint8_t)(a.table_u >> (56 - 8 * i));
            dst[9] = (uint8_t)'_';
            dst[10] = (uint8_t)'i';
            for (int i = 0; i < 8; i++) dst[11 + i] = (uint8_t)(a.index_u >> (56 - 8 * i));
            pos = 19;
        }
        for (int k = 0; k < n_cols; k++) {  // every lane of the workgroup walks the columns together
            const bool nn = live && wenc_notnull(a.c, k, r);
            if (live && !nn) dst[pos++] = 0;  // NilFlag
            if (a.c.type[k] != TSQ_BYTES) {   // uniform
                if (nn) {
                    uint64_t lo;
                    uint32_t hi;
                    const uint32_t n = tsq_enc_bytes(a.c.type[k], true, wenc_load(a.c, k, r), true, &lo, &hi);
                    wenc_put_datum(dst + pos, lo, hi, n);
                    pos += n;
                }
                continue;
            }
            // bytesFlag + the groups of 8 bytes with their markers
            int64_t s0 = 0;
            uint64_t n = 0, m8 = 0;
            const uint8_t* col = (const uint8_t*)a.c.data[k];
            if (nn) {
                s0 = a.c.offs[k][r];
                bool bad;
                n = ienc_cell_len(a, k, s0, (uint64_t)(a.c.offs[k][r + 1] - s0), &bad);
                m8 = tsq_enc_membytes_len(n) - 1u;
                dst[pos++] = 1;
            }
            const bool by_wave = nn && n >= (uint64_t)a.s.wave_copy_min;
            if (nn && !by_wave) {
                for (uint64_t i = 0; i < m8; i++) dst[pos + i] = tsq_enc_membytes_at(col + s0, n, i);
            }
            unsigned long long m = __ballot(by_wave);
            const uint64_t my_at = (staged ? (uint64_t)skew : (uint64_t)base) + ex + pos;  // into img | into keys
            while (m) {
                const int l = __ffsll(m) - 1;
                m &= m - 1;
                const uint64_t at = __shfl((unsigned long long)my_at, l, 64), cn = __shfl((unsigned long long)n, l, 64);
                const int64_t cs = (int64_t)__shfl((unsigned long long)s0, l, 64);
                const uint64_t cm = tsq_enc_membytes_len(cn) - 1u;
                uint8_t* d = staged ? img + at : a.keys + at;
                for (uint64_t i = lane; i < cm; i += 64) d[i] = tsq_enc_membytes_at(col + cs, cn, i);
            }
            pos += m8;
        }
        if (live && !w.distinct) {
            uint64_t lo;
            uint32_t hi;
            const uint32_t n = tsq_enc_bytes(TSQ_I64, true, (uint64_t)handle, true, &lo, &hi);
            wenc_put_datum(dst + pos, lo, hi, n);
        }
        __syncthreads();
        if (staged) wenc_copy_out(a.keys, base, plan, s_img);
        __syncthreads();
        base += (int64_t)T;
        vbase += (int64_t)vT;
    }
    if (tid == 0 && t1 == a.s.n_tiles && t1 > t0) {  // the workgroup that owns the last tile
        a.key_offsets[a.s.nrows] = base;
        a.value_offsets[a.s.nrows] = vbase;
    }
}

// ====================================================================== host side
struct WencStage {  // device copies of host columns
    DevBuf data[TSQ_MAX_COLS], bm[TSQ_MAX_COLS], co[TSQ_MAX_COLS];
};

// argument checks shared by the two entry points; *in_dev: the columns are TSQ_COL_DEVICE
tsq_status wenc_check_cols(tsq_handle_hdr* h, const char* fn, const tsq_col* cols, int32_t n_cols, int64_t nrows, bool* in_dev) {
    const std::string f(fn);
    bool dev = false, host = false;
    for (int c = 0; c < n_cols; c++) {
        if (cols[c].type < TSQ_I64 || cols[c].type > TSQ_BYTES) return tsq_fail(h, TSQ_ERR_INVALID, f + ": unknown column type");
        if (cols[c].length < nrows) return tsq_fail(h, TSQ_ERR_INVALID, f + ": column shorter than nrows");
        if (cols[c].type == TSQ_BYTES) {
            if (nrows > 0 && !cols[c].offsets) return tsq_fail(h, TSQ_ERR_INVALID, f + ": var-len column without offsets");
        } else if (nrows > 0 && !cols[c].data) {
            return tsq_fail(h, TSQ_ERR_INVALID, f + ": column data == NULL");
        }
        (cols[c].flags & TSQ_COL_DEVICE) ? dev = true : host = true;
    }
    if (dev && host) return tsq_fail(h, TSQ_ERR_INVALID, f + ": mixed host/device columns");
    *in_dev = dev;
    return TSQ_OK;
}

// the columns as the kernels read them: device columns as they are, host columns through a staged copy
tsq_status wenc_stage_cols(tsq_ctx* ctx, const char* fn, const tsq_col* cols, int32_t n_cols, int64_t nrows, bool in_dev, WencStage& st, WencCols& wc) {
    tsq_handle_hdr* h = &ctx->hdr;
    wc.n_cols = n_cols;
    tsq_status s = TSQ_OK;
    hipError_t e = hipSuccess;
    for (int c = 0; c < n_cols && s == TSQ_OK && e == hipSuccess; c++) {
        wc.type[c] = cols[c].type;
        const bool var = cols[c].type == TSQ_BYTES;
        if (in_dev) {
            wc.data[c] = cols[c].data;
            wc.nulls[c] = cols[c].null_bitmap;
            wc.offs[c] = var ? cols[c].offsets : nullptr;
            continue;
        }
        if (var) {  // its offsets and the bytes they span (the offsets may start anywhere: the kernels index data with them)
            const int64_t b0 = cols[c].offsets[0], b1 = cols[c].offsets[nrows];
            if (b1 < b0) return tsq_fail(h, TSQ_ERR_INVALID, std::string(fn) + ": var-len column: offsets must not decrease");
            s = st.co[c].reserve(ctx, h, ((size_t)nrows + 1) * 8 + 64);
            if (s == TSQ_OK) s = st.data[c].reserve(ctx, h, (size_t)(b1 - b0) + 64);
            if (s == TSQ_OK) e = hipMemcpyAsync(st.co[c].p, cols[c].offsets, ((size_t)nrows + 1) * 8, hipMemcpyHostToDevice, ctx->stream);
            if (s == TSQ_OK && e == hipSuccess && b1 > b0) e = hipMemcpyAsync(st.data[c].p, (const uint8_t*)cols[c].data + b0, (size_t)(b1 - b0), hipMemcpyHostToDevice, ctx->stream);
            wc.data[c] = (const uint8_t*)st.data[c].p - b0;  // data[offsets[r]] addresses the staged copy
            wc.offs[c] = st.co[c].as<int64_t>();
        } else {
            const size_t es = (size_t)tsq_elem_size(cols[c].type);
            s = st.data[c].reserve(ctx, h, (size_t)nrows * es + 64);
            if (s == TSQ_OK) e = hipMemcpyAsync(st.data[c].p, cols[c].data, (size_t)nrows * es, hipMemcpyHostToDevice, ctx->stream);
            wc.data[c] = st.data[c].p;
        }
        if (s == TSQ_OK && e == hipSuccess && cols[c].null_bitmap) {
            s = st.bm[c].reserve(ctx, h, tsq_bitmap_bytes(nrows) + 64);
            if (s == TSQ_OK) e = hipMemcpyAsync(st.bm[c].p, cols[c].null_bitmap, tsq_bitmap_bytes(nrows), hipMemcpyHostToDevice, ctx->stream);
            wc.nulls[c] = st.bm[c].as<uint8_t>();
        }
    }
    TSQ_TRY(s);
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string(fn) + "(H2D): " + hipGetErrorString(e));
    return TSQ_OK;
}

void wenc_shape(const tsq_ctx* ctx, int64_t nrows, WencShape& s) {
    s.nrows = nrows;
    s.n_tiles = (nrows + WENC_NT - 1) / WENC_NT;
    // workgroup b owns tiles [b * R, (b + 1) * R): <= 1024 workgroups, up to 8 per CU
    const int64_t want = std::min<int64_t>(std::min<int64_t>(s.n_tiles, (int64_t)ctx->num_cus * 8), WENC_MAXWG);
    s.tiles_per_wg = (s.n_tiles + want - 1) / want;
    s.n_wg = (int32_t)((s.n_tiles + s.tiles_per_wg - 1) / s.tiles_per_wg);
    const int64_t k = tsq_knob(ctx, TSQ_KNOB_ROWENC_WAVE_COPY, WENC_WAVE_COPY_DEFAULT);
    s.wave_copy_min = k <= 0 ? 0xffffffffu : (uint32_t)std::min<int64_t>(k, 0xffffffffLL);
}

// the LDS image of a launch whose rows are at most row_max bytes (var-len cells counted with a guess: tiles that do not fit go direct)
uint32_t wenc_lds_bytes(size_t row_max, bool any_var) {
    size_t lds = (((size_t)WENC_NT * row_max + 15 + 16 + 15) / 16) * 16;  // the tile at any skew, whole vectors
    if (any_var) lds = std::max<size_t>(lds, 32 * 1024);
    return (uint32_t)std::min<size_t>(lds, 60 * 1024);  // + the static words: within the 64 KiB a workgroup may ask for
}

}  // namespace

TSQ_API tsq_status tsq_rowcodec_encode(tsq_ctx* ctx, const tsq_col* cols, int32_t n_cols, const int64_t* col_ids, const uint32_t* col_flags, int64_t nrows,
                                       uint8_t* out, int64_t cap_bytes, uint32_t out_flags, int64_t* row_offsets, int64_t* bytes_out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (bytes_out) *bytes_out = 0;
    if (!bytes_out || !cols || !col_ids || nrows < 0 || cap_bytes < 0 || (cap_bytes > 0 && !out)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rowcodec_encode: bad arguments");
    if (n_cols < 1 || n_cols > TSQ_MAX_COLS) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rowcodec_encode: 1..16 columns supported");
    bool in_dev = false;
    tsq_status s = wenc_check_cols(h, "tsq_rowcodec_encode", cols, n_cols, nrows, &in_dev);
    TSQ_TRY(s);
    RencArgs a;
    memset(&a, 0, sizeof a);
    size_t row_max = 6;
    bool any_var = false;
    for (int c = 0; c < n_cols; c++) {
        if (col_ids[c] < 0 || col_ids[c] > 0xffffffffLL) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rowcodec_encode: a column id outside [0, 2^32)");
        for (int d = 0; d < c; d++) {
            if (col_ids[d] == col_ids[c]) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rowcodec_encode: duplicate column id");
        }
        a.ids[c] = (uint32_t)col_ids[c];
        if (col_ids[c] > 255) a.id_large = 1;
        const bool bit = col_flags && (col_flags[c] & TSQ_RC_BIT);
        if (bit) {
            if (cols[c].type != TSQ_BYTES) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rowcodec_encode: TSQ_RC_BIT on a column that is not TSQ_BYTES");
            a.bit_mask |= 1u << c;
        }
        const bool var = cols[c].type == TSQ_BYTES && !bit;
        any_var = any_var || var;
        row_max += var ? 32u : 8u;  // (strings: a guess)
    }
    row_max += (size_t)n_cols * (a.id_large ? 8u : 3u);
    // the id order of the columns: the same for every row (reformatCols sorts each row's not-null and null parts by id)
    for (int c = 0; c < n_cols; c++) a.perm[c] = (uint8_t)c;
    std::sort(a.perm, a.perm + n_cols, [&](uint8_t x, uint8_t y) { return a.ids[x] < a.ids[y]; });
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool out_dev = out_flags & TSQ_COL_DEVICE;
    if (nrows == 0) {  // no rows: the first row boundary
        if (row_offsets) {
            if (out_dev) TSQ_HIP(h, hipMemsetAsync(row_offsets, 0, sizeof(row_offsets[0]), ctx->stream));
            else row_offsets[0] = 0;
        }
        return TSQ_OK;
    }
    wenc_shape(ctx, nrows, a.s);
    WencStage st;
    DevBuf dwg, dout, doffs;
    s = dwg.reserve(ctx, h, ((size_t)a.s.n_wg + 1) * 8 + 64 + 64);
    if (s == TSQ_OK) s = wenc_stage_cols(ctx, "tsq_rowcodec_encode", cols, n_cols, nrows, in_dev, st, a.c);
    TSQ_TRY(s);
    a.s.wg_bytes = dwg.as<unsigned long long>();
    a.s.err = (uint32_t*)(a.s.wg_bytes + a.s.n_wg + 1);
    // pass 1 + scan: the size of the byte string is known before a byte is written
    hipError_t e = hipMemsetAsync(a.s.err, 0, 8, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_renc_size, dim3(a.s.n_wg), dim3(WENC_NT), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_wenc_scan, dim3(1), dim3(64), 0, ctx->stream, a.s, 1);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned, a.s.wg_bytes + a.s.n_wg, 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_rowcodec_encode: ") + hipGetErrorString(e));
    const int64_t total = (int64_t)ctx->pinned[0];
    const uint64_t errw = ctx->pinned[1];
    if ((uint32_t)errw) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rowcodec_encode: a bit column's cell is not 1..8 bytes long");
    if (errw >> 32) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_rowcodec_encode: a row's values reach 4 GiB");
    *bytes_out = total;
    if (total > cap_bytes) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rowcodec_encode: output buffer too small (*bytes_out = bytes needed)");
    if (out_dev) {
        a.out = out;
        a.row_offsets = row_offsets;
    } else {
        s = dout.reserve(ctx, h, (size_t)total + 64);
        if (s == TSQ_OK && row_offsets) s = doffs.reserve(ctx, h, ((size_t)nrows + 1) * 8 + 64);
        TSQ_TRY(s);
        a.out = dout.as<uint8_t>();
        a.row_offsets = row_offsets ? doffs.as<int64_t>() : nullptr;
    }
    a.s.lds_bytes = wenc_lds_bytes(row_max, any_var);
    hipLaunchKernelGGL(k_renc_emit, dim3(a.s.n_wg), dim3(WENC_NT), a.s.lds_bytes, ctx->stream, a);
    e = hipGetLastError();
    if (e == hipSuccess && !out_dev) {
        if (total > 0) e = hipMemcpyAsync(out, a.out, (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && row_offsets) e = hipMemcpyAsync(row_offsets, a.row_offsets, ((size_t)nrows + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_rowcodec_encode: ") + hipGetErrorString(e));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_indexkeys_encode(tsq_ctx* ctx, int64_t table_id, int64_t index_id, uint32_t index_flags, const tsq_col* cols, int32_t n_index_cols,
                                        const int32_t* prefix_len, const uint8_t* prefix_utf8, const int64_t* handles, int64_t nrows, uint32_t data_flags,
                                        uint8_t* keys_out, int64_t cap_bytes, int64_t* key_offsets, uint8_t* values_out, int64_t* value_offsets,
                                        uint8_t* distinct_out, int64_t* bytes_out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (bytes_out) *bytes_out = 0;
    if (!bytes_out || !cols || nrows < 0 || cap_bytes < 0 || (cap_bytes > 0 && !keys_out) || !key_offsets || !value_offsets || (nrows > 0 && !handles))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_indexkeys_encode: bad arguments");
    if (n_index_cols < 1 || n_index_cols > TSQ_MAX_COLS) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_indexkeys_encode: 1..16 index columns supported");
    bool in_dev = false;
    tsq_status s = wenc_check_cols(h, "tsq_indexkeys_encode", cols, n_index_cols, nrows, &in_dev);
    TSQ_TRY(s);
    IencArgs a;
    memset(&a, 0, sizeof a);
    size_t row_max = 19 + 9;
    bool any_var = false;
    for (int c = 0; c < n_index_cols; c++) {
        const bool var = cols[c].type == TSQ_BYTES;
        a.prefix_len[c] = (var && prefix_len && prefix_len[c] >= 0) ? prefix_len[c] : -1;
        if (var && prefix_utf8 && prefix_utf8[c]) a.utf8_mask |= 1u << c;
        any_var = any_var || var;
        row_max += var ? 40u : 9u;  // (strings: a guess)
    }
    a.unique = (index_flags & TSQ_IDX_UNIQUE) ? 1u : 0u;
    a.table_u = (uint64_t)table_id ^ 0x8000000000000000ULL;
    a.index_u = (uint64_t)index_id ^ 0x8000000000000000ULL;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool out_dev = data_flags & TSQ_COL_DEVICE;
    if (nrows == 0) {
        if (out_dev) {
            TSQ_HIP(h, hipMemsetAsync(key_offsets, 0, sizeof(key_offsets[0]), ctx->stream));
            TSQ_HIP(h, hipMemsetAsync(value_offsets, 0, sizeof(value_offsets[0]), ctx->stream));
        } else {
            key_offsets[0] = value_offsets[0] = 0;
        }
        return TSQ_OK;
    }
    wenc_shape(ctx, nrows, a.s);
    WencStage st;
    DevBuf dwg, dh, dkeys, dko, dvals, dvo, ddist;
    s = dwg.reserve(ctx, h, 2 * ((size_t)a.s.n_wg + 1) * 8 + 64 + 64);
    if (s == TSQ_OK) s = wenc_stage_cols(ctx, "tsq_indexkeys_encode", cols, n_index_cols, nrows, in_dev, st, a.c);
    hipError_t e = hipSuccess;
    if (s == TSQ_OK) {  // the handles live where the columns live
        if (in_dev) {
            a.handles = handles;
        } else {
            s = dh.reserve(ctx, h, (size_t)nrows * 8 + 64);
            if (s == TSQ_OK) e = hipMemcpyAsync(dh.p, handles, (size_t)nrows * 8, hipMemcpyHostToDevice, ctx->stream);
            a.handles = dh.as<int64_t>();
        }
    }
    TSQ_TRY(s);
    a.s.wg_bytes = dwg.as<unsigned long long>();
    a.s.err = (uint32_t*)(a.s.wg_bytes + 2 * ((size_t)a.s.n_wg + 1));
    if (e == hipSuccess) e = hipMemsetAsync(a.s.err, 0, 8, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_ienc_size, dim3(a.s.n_wg), dim3(WENC_NT), 0, ctx->stream, a);
        hipLaunchKernelGGL(k_wenc_scan, dim3(1), dim3(64), 0, ctx->stream, a.s, 2);
        e = hipGetLastError();
    }
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned, a.s.wg_bytes + a.s.n_wg, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned + 1, a.s.wg_bytes + 2 * (size_t)a.s.n_wg + 1, 16, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_indexkeys_encode: ") + hipGetErrorString(e));
    const int64_t total = (int64_t)ctx->pinned[0], vtotal = (int64_t)ctx->pinned[1];
    if (ctx->pinned[2] >> 32)
        return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_indexkeys_encode: invalid UTF-8 inside the kept prefix of a truncated cell (the reference rewrites it)");
    *bytes_out = total;
    if (total > cap_bytes) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_indexkeys_encode: output buffer too small (*bytes_out = bytes needed)");
    if (!values_out) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_indexkeys_encode: values_out == NULL");
    if (out_dev) {
        a.keys = keys_out;
        a.key_offsets = key_offsets;
        a.values = values_out;
        a.value_offsets = value_offsets;
        a.distinct = distinct_out;
    } else {
        s = dkeys.reserve(ctx, h, (size_t)total + 64);
        if (s == TSQ_OK) s = dko.reserve(ctx, h, ((size_t)nrows + 1) * 8 + 64);
        if (s == TSQ_OK) s = dvals.reserve(ctx, h, (size_t)nrows * 8 + 64);
        if (s == TSQ_OK) s = dvo.reserve(ctx, h, ((size_t)nrows + 1) * 8 + 64);
        if (s == TSQ_OK && distinct_out) s = ddist.reserve(ctx, h, (size_t)nrows + 64);
        TSQ_TRY(s);
        a.keys = dkeys.as<uint8_t>();
        a.key_offsets = dko.as<int64_t>();
        a.values = dvals.as<uint8_t>();
        a.value_offsets = dvo.as<int64_t>();
        a.distinct = distinct_out ? ddist.as<uint8_t>() : nullptr;
    }
    a.s.lds_bytes = wenc_lds_bytes(row_max, any_var);
    hipLaunchKernelGGL(k_ienc_emit, dim3(a.s.n_wg), dim3(WENC_NT), a.s.lds_bytes, ctx->stream, a);
    e = hipGetLastError();
    if (e == hipSuccess && !out_dev) {
        e = hipMemcpyAsync(keys_out, a.keys, (size_t)total, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(key_offsets, a.key_offsets, ((size_t)nrows + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(values_out, a.values, (size_t)vtotal, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipMemcpyAsync(value_offsets, a.value_offsets, ((size_t)nrows + 1) * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && distinct_out) e = hipMemcpyAsync(distinct_out, a.distinct, (size_t)nrows, hipMemcpyDeviceToHost, ctx->stream);
    }
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_indexkeys_encode: ") + hipGetErrorString(e));
    return TSQ_OK;
}
