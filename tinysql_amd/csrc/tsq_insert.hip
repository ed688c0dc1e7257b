// tsq_insert.hip — the per-row step of INSERT ... SELECT on the GPU (gfx950): the select's chunk -> the cells tables.AddRecord is
// handed (include/tsq.h "INSERT .. SELECT").  The per-cell arithmetic is tsq_insert_dp.h.
//
// tsq_cast_run:
//   K19a k_ins_cast_tpl<false> ("k_ins_cast_fixed" in the documents): ONE launch for every fixed-width column fed by a fixed-width one.  The column specs travel in the kernel arguments.
//                           A lane takes two neighbouring rows of a column with one 16-byte access (float32 cells: 8 bytes), so a
//                           wave reads and writes 1 KB of a column per instruction; the lane's two NOT-NULL bits meet those of its
//                           fifteen neighbours in a shuffle tree and the sixteenth lane writes one whole 32-row word of the bitmap.
//                           The rows behind the last whole 128-row step (and every row, when a buffer is not 16-byte aligned) go one
//                           row per lane; their bitmap bytes come from a ballot.  A failing cell is (row, phase, column, status) in one
//                           word: min inside the wave, then one 64-bit atomicMin; warnings are summed inside the wave before one
//                           atomicAdd per kind.  A wave whose rows are all fine touches no atomic.
// tsq_autoid_fill: the allocator state is a scan under f(x) = max(x + a, b) (tsq_insert_dp.h), three launches, no look-back spin —
// no workgroup ever waits for another one:
//   K19b k_aid_agg   : per 1024-row tile the composed operator, the first allocating row and the last explicit row
//   K19c k_aid_scan  : ONE workgroup: the tiles' operators -> the allocator state in front of every tile, the new base, the rows
//                      of the first allocation / last explicit id of the chunk
//   K19d k_aid_apply : per tile the scan inside the workgroup (wave steps as in tsq_wavescan.h, the wave totals through LDS), the
//                      ids written in place, the bitmap bytes set, the first id above the column type's bound by atomicMin
#include "tsq_stage.h"
#include "tsq_insert_dp.h"

#include <memory>

struct InsCastArgs {
    tsq_ins_col col[TSQ_MAX_COLS];
    const void* in_data[TSQ_MAX_COLS];     // by TABLE column; nullptr for a column that takes its default
    const uint8_t* in_null[TSQ_MAX_COLS];  // nullptr: no NULLs
    void* out_data[TSQ_MAX_COLS];
    uint8_t* out_null[TSQ_MAX_COLS];
    const int64_t* in_offs[TSQ_MAX_COLS];  // a TSQ_BYTES source: its offsets
    int64_t* lens[TSQ_MAX_COLS];           // a string target: the library's [nrows + 1] cell lengths, then (scan) the offsets
    int64_t* out_offs[TSQ_MAX_COLS];       // ... and the caller's offsets, written by the write pass
    const uint8_t* def_dev[TSQ_MAX_COLS];  // ... its default bytes in HBM
    int32_t n_cols;
    uint32_t stmt_flags;
    uint32_t str_ctx;  // TSQ_STRCTX_*: string -> integer
    int64_t nrows;
    int64_t n_vec;              // rows of the two-rows-per-lane part: a multiple of 128, 0 when a buffer is not aligned for it
    int64_t bitmap_bytes;       // (nrows + 7) / 8
    unsigned long long* err;    // the smallest error word (tsq_ins_errword)
    unsigned long long* warn;   // [0] overflow, [1] bad null, [2] data too long, [3] bad utf8, [4] truncated (string -> integer) warnings
};

struct InsAcc {
    uint64_t errw;
    uint32_t w_ovf, w_null, w_trunc;
};
__device__ __forceinline__ uint64_t ins_one(const InsCastArgs& a, int c, int64_t row, uint64_t bits, bool in_null, bool* out_null, InsAcc& acc) {
    int32_t status, phase;
    const uint64_t v = tsq_ins_cell(a.col[c], a.stmt_flags, bits, in_null, out_null, &status, &phase, &acc.w_ovf, &acc.w_null);
    if (status != 0) {
        const uint64_t w = tsq_ins_errword(row, phase, phase ? c : a.col[c].src_col, c, status);
        acc.errw = w < acc.errw ? w : acc.errw;
    }
    return v;
}

// ... the same for an integer column fed by a string column: the cell's bytes by its offsets
__device__ __forceinline__ uint64_t ins_one_str(const InsCastArgs& a, int c, int64_t row, bool in_null, bool* out_null, InsAcc& acc) {
    const uint8_t* p = nullptr;
    uint32_t n = 0;
    if (!in_null) {
        const int64_t o0 = a.in_offs[c][row], o1 = a.in_offs[c][row + 1];
        p = reinterpret_cast<const uint8_t*>(a.in_data[c]) + o0;
        n = o1 > o0 ? (uint32_t)(o1 - o0) : 0u;
    }
    int32_t status, phase;
    uint32_t warn[3] = {0u, 0u, 0u};
    const uint64_t v = tsq_ins_cell_str_int(a.col[c], a.stmt_flags, a.str_ctx, p, n, in_null, out_null, &status, &phase, warn);
    acc.w_ovf += warn[0];
    acc.w_null += warn[1];
    acc.w_trunc += warn[2];
    if (status != 0) {
        const uint64_t w = tsq_ins_errword(row, phase, phase ? c : a.col[c].src_col, c, status);
        acc.errw = w < acc.errw ? w : acc.errw;
    }
    return v;
}

// STR_SRC = false: K19a.  STR_SRC = true: K19g k_ins_cast_tpl<true>, the integer columns fed by a STRING column (types.StrToInt / StrToUint,
// then the range clip): one row per lane throughout (a.n_vec is ignored), a launch of its own so that the parser's registers do not
// lower the occupancy of the numeric kernel
template <bool STR_SRC>
__global__ void __launch_bounds__(256) k_ins_cast_tpl(InsCastArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    InsAcc acc{TSQ_INS_ERR_NONE, 0u, 0u, 0u};
    // rows 2 p, 2 p + 1 (n_vec / 2 is a multiple of 64: the trip count is wave uniform)
    const int64_t npairs = STR_SRC ? 0 : a.n_vec >> 1;
    for (int64_t p = tid; p < npairs; p += nthreads) {
#pragma unroll 1
        for (int c = 0; c < a.n_cols; c++) {
            if (a.col[c].kind == TSQ_INS_STR) continue;  // (k_ins_str)
            const bool has_src = a.col[c].src_col >= 0;
            if (has_src && a.col[c].src_type == TSQ_BYTES) continue;  // (k_ins_str_int: the parser would halve this kernel's occupancy)
            uint64_t x0 = 0, x1 = 0;
            uint32_t nn = 3u;
            if (has_src) {
                if (a.col[c].src_type == TSQ_F32) {
                    const uint2 v = reinterpret_cast<const uint2*>(a.in_data[c])[p];
                    x0 = v.x;
                    x1 = v.y;
                } else {
                    const ulonglong2 v = reinterpret_cast<const ulonglong2*>(a.in_data[c])[p];
                    x0 = v.x;
                    x1 = v.y;
                }
                if (a.in_null[c]) nn = ((uint32_t)a.in_null[c][p >> 2] >> (2u * (uint32_t)(p & 3))) & 3u;
            }
            bool n0, n1;
            const uint64_t y0 = ins_one(a, c, 2 * p, x0, !(nn & 1u), &n0, acc);
            const uint64_t y1 = ins_one(a, c, 2 * p + 1, x1, !(nn & 2u), &n1, acc);
            if (a.col[c].out_f32) {
                reinterpret_cast<uint2*>(a.out_data[c])[p] = make_uint2((uint32_t)y0, (uint32_t)y1);
            } else {
                reinterpret_cast<ulonglong2*>(a.out_data[c])[p] = make_ulonglong2(y0, y1);
            }
            uint32_t w = ((n0 ? 0u : 1u) | (n1 ? 0u : 2u)) << (2u * (uint32_t)(lane & 15));
            w |= (uint32_t)__shfl_xor((int)w, 1, 64);
            w |= (uint32_t)__shfl_xor((int)w, 2, 64);
            w |= (uint32_t)__shfl_xor((int)w, 4, 64);
            w |= (uint32_t)__shfl_xor((int)w, 8, 64);
            if ((lane & 15) == 0) reinterpret_cast<uint32_t*>(a.out_null[c])[p >> 4] = w;  // rows 2 p .. 2 p + 31: word p / 16
        }
    }
    // the rest: one row per lane, 64 rows per wave step (n_vec is a multiple of 64: a step starts on a byte of the bitmaps)
    const int64_t wave = tid >> 6, nwaves = nthreads >> 6;
    for (int64_t r0 = (STR_SRC ? 0 : a.n_vec) + wave * 64; r0 < a.nrows; r0 += nwaves * 64) {
        const int64_t r = r0 + lane;
        const bool in = r < a.nrows;
#pragma unroll 1
        for (int c = 0; c < a.n_cols; c++) {
            if (a.col[c].kind == TSQ_INS_STR) continue;
            if ((a.col[c].src_col >= 0 && a.col[c].src_type == TSQ_BYTES) != STR_SRC) continue;
            bool on = true;
            if (in) {
                uint64_t x = 0;
                bool in_null = false;
                if (a.col[c].src_col >= 0) {
                    if (STR_SRC) x = 0;
                    else if (a.col[c].src_type == TSQ_F32) x = reinterpret_cast<const uint32_t*>(a.in_data[c])[r];
                    else x = reinterpret_cast<const uint64_t*>(a.in_data[c])[r];
                    in_null = tsq_is_null(a.in_null[c], r);
                }
                const uint64_t y = STR_SRC ? ins_one_str(a, c, r, in_null, &on, acc) : ins_one(a, c, r, x, in_null, &on, acc);
                if (a.col[c].out_f32) reinterpret_cast<uint32_t*>(a.out_data[c])[r] = (uint32_t)y;
                else reinterpret_cast<uint64_t*>(a.out_data[c])[r] = y;
            }
            const unsigned long long bal = __ballot(in && !on);
            const int64_t by = (r0 >> 3) + lane;
            if (lane < 8 && by < a.bitmap_bytes) a.out_null[c][by] = (uint8_t)(bal >> (8 * lane));
        }
    }
    // (rows without trouble: no shuffle tree, no atomic)
    if (__any(acc.errw != TSQ_INS_ERR_NONE)) {
        uint64_t m = acc.errw;
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t y = __shfl_xor(m, o, 64);
            m = y < m ? y : m;
        }
        if (lane == 0) atomicMin(a.err, (unsigned long long)m);
    }
    if (__any((acc.w_ovf | acc.w_null | acc.w_trunc) != 0u)) {
        uint32_t s0 = acc.w_ovf, s1 = acc.w_null, s2 = acc.w_trunc;
        for (int o = 32; o > 0; o >>= 1) {
            s0 += (uint32_t)__shfl_xor((int)s0, o, 64);
            s1 += (uint32_t)__shfl_xor((int)s1, o, 64);
            s2 += (uint32_t)__shfl_xor((int)s2, o, 64);
        }
        if (lane == 0) {
            if (s0) atomicAdd(a.warn, (unsigned long long)s0);
            if (s1) atomicAdd(a.warn + 1, (unsigned long long)s1);
            if (s2) atomicAdd(a.warn + 4, (unsigned long long)s2);
        }
    }
}

// K19e / K19f k_ins_str<false / true>: the string columns of the table, one row per lane, 64 rows per wave step.
//   <false> the length pass: every cell's shape (tsq_ins_str_cell) -> its length in `lens`, the errors and warnings of the run;
//           nothing of the caller's is written, so a sizing call (cap_bytes = 0) leaves the outputs untouched
//   (tsq_launch_scan64: lengths -> offsets + the total)
//   <true>  the write pass: offsets, NOT-NULL bits (ballot), the kept bytes and the zero padding of BINARY(n); a cell of 64 bytes or
//           more is copied by the whole wave, consecutive lanes on consecutive bytes (as tsq_rowcodec_encode, TSQ_KNOB_ROWENC_WAVE_COPY)
// A formatted integer (at most 20 bytes) lives in three registers.
template <bool WRITE>
__global__ void __launch_bounds__(256) k_ins_str(InsCastArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t tid = (int64_t)blockIdx.x * 256 + threadIdx.x, nthreads = (int64_t)gridDim.x * 256;
    const int64_t wave = tid >> 6, nwaves = nthreads >> 6;
    uint64_t errw = TSQ_INS_ERR_NONE;
    uint32_t warn[4] = {0u, 0u, 0u, 0u};
    for (int64_t r0 = wave * 64; r0 < a.nrows; r0 += nwaves * 64) {  // (wave uniform)
        const int64_t r = r0 + lane;
        const bool in = r < a.nrows;
#pragma unroll 1
        for (int c = 0; c < a.n_cols; c++) {
            if (a.col[c].kind != TSQ_INS_STR) continue;
            const bool has_src = a.col[c].src_col >= 0, src_bytes = a.col[c].src_type == TSQ_BYTES;
            const uint8_t* s = nullptr;
            uint64_t n = 0, w0 = 0, w1 = 0, w2 = 0;
            bool in_null = false;
            if (in && has_src) {
                in_null = tsq_is_null(a.in_null[c], r);
                if (!in_null) {
                    if (src_bytes) {
                        const int64_t o0 = a.in_offs[c][r], o1 = a.in_offs[c][r + 1];
                        s = reinterpret_cast<const uint8_t*>(a.in_data[c]) + o0;
                        n = o1 > o0 ? (uint64_t)(o1 - o0) : 0;
                    } else {
                        n = tsq_ins_format_int(a.col[c].src_type, reinterpret_cast<const uint64_t*>(a.in_data[c])[r], &w0, &w1, &w2);
                    }
                }
            }
            if (!WRITE) {
                if (in) {
                    uint64_t keep, pad;
                    bool from_default, on;
                    int32_t status, phase;
                    tsq_ins_str_cell(a.col[c], a.stmt_flags, s, n, in_null, &keep, &pad, &from_default, &on, &status, &phase, warn);
                    if (status != 0) {
                        const uint64_t w = tsq_ins_errword(r, phase, phase ? c : a.col[c].src_col, c, status);
                        errw = w < errw ? w : errw;
                    }
                    a.lens[c][r] = (status != 0 || on) ? 0 : (int64_t)(keep + pad);
                }
                continue;
            }
            // the write pass: the cell is `total` bytes at `off`: the first min(total, n) from the source, zeros behind them
            int64_t off = 0, total = 0;
            bool is_null = true;
            if (in) {
                off = a.lens[c][r];
                total = a.lens[c][r + 1] - off;
                a.out_offs[c][r] = off;
                if (r == a.nrows - 1) a.out_offs[c][a.nrows] = off + total;
                const bool src_null = has_src ? in_null : (a.col[c].flags & TSQ_CAST_DEFAULT_NULL) != 0;
                is_null = src_null && !((a.col[c].flags & TSQ_CAST_NOT_NULL) && (a.stmt_flags & TSQ_CAST_BAD_NULL_AS_WARNING));
                if (!has_src && !src_null) {
                    s = a.def_dev[c];
                    n = (uint64_t)a.col[c].def_len;
                }
            }
            const bool by_ptr = !has_src || src_bytes;
            const int64_t keep = total < (int64_t)n ? total : (int64_t)n;
            uint8_t* d = reinterpret_cast<uint8_t*>(a.out_data[c]) + off;
            const bool by_wave = by_ptr && total >= 64;
            if (in && total > 0 && !by_wave) {
                if (by_ptr) {
                    if (keep > 0) tsq_copy_cell(d, s, keep);
                } else {
                    for (int64_t i = 0; i < keep; i++) d[i] = tsq_ins_fmt_byte(w0, w1, w2, (uint32_t)i);
                }
                for (int64_t i = keep; i < total; i++) d[i] = 0;
            }
            unsigned long long todo = __ballot(in && by_wave);
            while (todo) {  // (wave uniform)
                const int src_lane = __ffsll((long long)todo) - 1;
                todo &= todo - 1;
                const uint8_t* ws = (const uint8_t*)__shfl((unsigned long long)s, src_lane, 64);
                uint8_t* wd = (uint8_t*)__shfl((unsigned long long)d, src_lane, 64);
                const int64_t wk = (int64_t)__shfl((unsigned long long)keep, src_lane, 64), wt = (int64_t)__shfl((unsigned long long)total, src_lane, 64);
                for (int64_t b = lane; b < wt; b += 64) wd[b] = b < wk ? ws[b] : (uint8_t)0;
            }
            const unsigned long long bal = __ballot(in && !is_null);
            const int64_t by = (r0 >> 3) + lane;
            if (lane < 8 && by < a.bitmap_bytes) a.out_null[c][by] = (uint8_t)(bal >> (8 * lane));
        }
    }
    if (!WRITE) {
        if (__any(errw != TSQ_INS_ERR_NONE)) {
            uint64_t m = errw;
            for (int o = 32; o > 0; o >>= 1) {
                const uint64_t y = __shfl_xor(m, o, 64);
                m = y < m ? y : m;
            }
            if (lane == 0) atomicMin(a.err, (unsigned long long)m);
        }
        if (__any((warn[0] | warn[1] | warn[2] | warn[3]) != 0u)) {
#pragma unroll
            for (int k = 1; k < 4; k++) {
                uint32_t v = warn[k];
                for (int o = 32; o > 0; o >>= 1) v += (uint32_t)__shfl_xor((int)v, o, 64);
                if (lane == 0 && v) atomicAdd(a.warn + k, (unsigned long long)v);
            }
        }
    }
}

// ====================================================================== auto ids
#define TSQ_AID_TILE 1024  // rows per workgroup: 256 threads x 4 neighbouring rows
// result words of the scan
#define AID_R_NEW_BASE 0
#define AID_R_FIRST_ROW 1   // row of the first allocation, INT64_MAX: none
#define AID_R_LAST_ROW 2    // row of the last explicit id, -1: none
#define AID_R_OVF 3
#define AID_R_ERR_ROW 4     // atomicMin, all ones: none
#define AID_R_FIRST_VAL 5
#define AID_R_LAST_VAL 6

struct AidArgs {
    int64_t* data;
    uint8_t* nulls;       // nullptr: no NULLs (and nothing to rewrite)
    int64_t n, base, upper;
    uint32_t flags;
    int32_t vec;          // data is 16-byte aligned
    int64_t n_tiles;
    tsq_aid_op* agg;      // [n_tiles]
    int64_t* tile_first;  // [n_tiles] first allocating row of the tile, INT64_MAX: none
    int64_t* tile_last;   // [n_tiles] last explicit row, -1: none
    int64_t* s_in;        // [n_tiles] allocator state in front of the tile
    unsigned long long* res;
};

__device__ __forceinline__ tsq_aid_op aid_shfl_up(const tsq_aid_op& x, int o) {
    tsq_aid_op y;
    y.a = (int64_t)__shfl_up((uint64_t)x.a, o, 64);
    y.b = (int64_t)__shfl_up((uint64_t)x.b, o, 64);
    y.ovf = __shfl_up(x.ovf, o, 64);
    return y;
}
// inclusive scan over the lanes of a wave (lanes hold consecutive stretches; the operator does not commute)
__device__ __forceinline__ tsq_aid_op aid_wave_scan(tsq_aid_op x, int lane) {
    for (int k = 0; k < 6; k++) {
        const tsq_aid_op y = aid_shfl_up(x, 1 << k);
        if (lane >= (1 << k)) x = tsq_aid_compose(y, x);
    }
    return x;
}
// a thread's four rows: values, kinds (rows at or behind n: TSQ_AID_KEEP)
__device__ __forceinline__ void aid_load4(const AidArgs& a, int64_t row0, int64_t (&v)[4], int (&kind)[4]) {
    uint32_t nn = 0xfu;
    if (a.nulls && row0 < a.n) nn = ((uint32_t)a.nulls[row0 >> 3] >> (uint32_t)(row0 & 4)) & 0xfu;
    if (a.vec && row0 + 4 <= a.n) {
        const ulonglong2 p = reinterpret_cast<const ulonglong2*>(a.data + row0)[0], q = reinterpret_cast<const ulonglong2*>(a.data + row0)[1];
        v[0] = (int64_t)p.x;
        v[1] = (int64_t)p.y;
        v[2] = (int64_t)q.x;
        v[3] = (int64_t)q.y;
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++) v[i] = row0 + i < a.n ? a.data[row0 + i] : 0;
    }
#pragma unroll
    for (int i = 0; i < 4; i++) kind[i] = row0 + i < a.n ? tsq_aid_row_kind(v[i], !((nn >> i) & 1u), a.flags) : TSQ_AID_KEEP;
}
// returns the composed operator of the workgroup's whole tile to EVERY thread; with `excl` given, *excl = the operator of everything
// in the tile in front of this thread (the exclusive scan).  Two barriers: s_wave may be reused right after the call
__device__ __forceinline__ tsq_aid_op aid_block_scan(tsq_aid_op mine, tsq_aid_op* excl, tsq_aid_op* s_wave) {
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6, nw = blockDim.x >> 6;
    const tsq_aid_op inc = aid_wave_scan(mine, lane);
    if (lane == 63) s_wave[w] = inc;
    __syncthreads();
    tsq_aid_op before = tsq_aid_identity(), total = tsq_aid_identity();
    for (int i = 0; i < nw; i++) {  // (at most 16 waves)
        if (i == w) before = total;
        total = tsq_aid_compose(total, s_wave[i]);
    }
    if (excl) {
        tsq_aid_op up = aid_shfl_up(inc, 1);
        if (lane == 0) up = tsq_aid_identity();
        *excl = tsq_aid_compose(before, up);
    }
    __syncthreads();
    return total;
}

__global__ void __launch_bounds__(256) k_aid_agg(AidArgs a) {
    __shared__ tsq_aid_op s_wave[4];
    __shared__ int64_t s_first[4], s_last[4];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t row0 = (int64_t)blockIdx.x * TSQ_AID_TILE + (int64_t)threadIdx.x * 4;
    int64_t v[4];
    int kind[4];
    aid_load4(a, row0, v, kind);
    tsq_aid_op mine = tsq_aid_identity();
    int64_t first = TSQ_I64MAX, last = -1;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        mine = tsq_aid_compose(mine, tsq_aid_row_op(kind[i], v[i]));
        if (kind[i] == TSQ_AID_ALLOC && first == TSQ_I64MAX) first = row0 + i;
        if (kind[i] == TSQ_AID_EXPLICIT) last = row0 + i;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t f = (int64_t)__shfl_xor((uint64_t)first, o, 64), l = (int64_t)__shfl_xor((uint64_t)last, o, 64);
        first = f < first ? f : first;
        last = l > last ? l : last;
    }
    if (lane == 0) {
        s_first[w] = first;
        s_last[w] = last;
    }
    const tsq_aid_op total = aid_block_scan(mine, nullptr, s_wave);
    if (threadIdx.x == 0) {
        for (int i = 0; i < 4; i++) {
            first = s_first[i] < first ? s_first[i] : first;
            last = s_last[i] > last ? s_last[i] : last;
        }
        a.agg[blockIdx.x] = total;
        a.tile_first[blockIdx.x] = first;
        a.tile_last[blockIdx.x] = last;
    }
}

__global__ void __launch_bounds__(1024) k_aid_scan(AidArgs a) {
    __shared__ tsq_aid_op s_wave[16];
    __shared__ int64_t s_first[16], s_last[16];
    const int lane = threadIdx.x & 63, w = threadIdx.x >> 6;
    const int64_t per = (a.n_tiles + 1023) / 1024;
    const int64_t lo = (int64_t)threadIdx.x * per;
    int64_t hi = lo + per;
    hi = hi < a.n_tiles ? hi : a.n_tiles;
    tsq_aid_op mine = tsq_aid_identity();
    int64_t first = TSQ_I64MAX, last = -1;
    for (int64_t i = lo; i < hi; i++) {
        mine = tsq_aid_compose(mine, a.agg[i]);
        const int64_t f = a.tile_first[i], l = a.tile_last[i];
        first = f < first ? f : first;
        last = l > last ? l : last;
    }
    for (int o = 32; o > 0; o >>= 1) {
        const int64_t f = (int64_t)__shfl_xor((uint64_t)first, o, 64), l = (int64_t)__shfl_xor((uint64_t)last, o, 64);
        first = f < first ? f : first;
        last = l > last ? l : last;
    }
    if (lane == 0) {
        s_first[w] = first;
        s_last[w] = last;
    }
    tsq_aid_op run;
    const tsq_aid_op total = aid_block_scan(mine, &run, s_wave);
    int32_t ovf = 0;
    for (int64_t i = lo; i < hi; i++) {
        a.s_in[i] = tsq_aid_apply(run, a.base, &ovf);
        run = tsq_aid_compose(run, a.agg[i]);
    }
    if (threadIdx.x == 0) {
        for (int i = 0; i < 16; i++) {
            first = s_first[i] < first ? s_first[i] : first;
            last = s_last[i] > last ? s_last[i] : last;
        }
        int32_t o2 = 0;
        a.res[AID_R_NEW_BASE] = (unsigned long long)tsq_aid_apply(total, a.base, &o2);
        a.res[AID_R_FIRST_ROW] = (unsigned long long)first;
        a.res[AID_R_LAST_ROW] = (unsigned long long)last;
        a.res[AID_R_OVF] = (unsigned long long)o2;  // (an overflow in front of a tile is one of the whole chunk too: s never decreases)
    }
}

__global__ void __launch_bounds__(256) k_aid_apply(AidArgs a) {
    __shared__ tsq_aid_op s_wave[4];
    const int lane = threadIdx.x & 63;
    const int64_t row0 = (int64_t)blockIdx.x * TSQ_AID_TILE + (int64_t)threadIdx.x * 4;
    int64_t v[4];
    int kind[4];
    aid_load4(a, row0, v, kind);
    tsq_aid_op mine = tsq_aid_identity();
#pragma unroll
    for (int i = 0; i < 4; i++) mine = tsq_aid_compose(mine, tsq_aid_row_op(kind[i], v[i]));
    tsq_aid_op before;
    (void)aid_block_scan(mine, &before, s_wave);
    int32_t ovf = 0;
    int64_t s = tsq_aid_apply(before, a.s_in[blockIdx.x], &ovf);
    const int64_t first_row = (int64_t)a.res[AID_R_FIRST_ROW], last_row = (int64_t)a.res[AID_R_LAST_ROW];
    uint64_t bad = ~0ull;
#pragma unroll
    for (int i = 0; i < 4; i++) {
        const int64_t r = row0 + i;
        if (kind[i] == TSQ_AID_EXPLICIT) {
            s = v[i] > s ? v[i] : s;
            if (r == last_row) a.res[AID_R_LAST_VAL] = (unsigned long long)v[i];
        } else if (kind[i] == TSQ_AID_ALLOC) {
            if (s == TSQ_I64MAX) ovf = 1;
            else s += 1;
            v[i] = s;
            if (s > a.upper && bad == ~0ull) bad = (uint64_t)r;
            if (r == first_row) a.res[AID_R_FIRST_VAL] = (unsigned long long)s;
        } else if (r < a.n) {
            v[i] = 0;  // a 0 that stays (a NULL never comes here)
        }
    }
    if (a.vec && row0 + 4 <= a.n) {
        reinterpret_cast<ulonglong2*>(a.data + row0)[0] = make_ulonglong2((uint64_t)v[0], (uint64_t)v[1]);
        reinterpret_cast<ulonglong2*>(a.data + row0)[1] = make_ulonglong2((uint64_t)v[2], (uint64_t)v[3]);
    } else {
#pragma unroll
        for (int i = 0; i < 4; i++)
            if (row0 + i < a.n) a.data[row0 + i] = v[i];
    }
    if (a.nulls) {  // every row is NOT NULL now: two threads make a byte (the bits behind the last row stay 0)
        int64_t left = a.n - row0;
        left = left < 0 ? 0 : (left > 4 ? 4 : left);
        uint32_t nib = (1u << left) - 1u;
        const uint32_t other = (uint32_t)__shfl_xor((int)nib, 1, 64);
        if (!(threadIdx.x & 1) && row0 < a.n) a.nulls[row0 >> 3] = (uint8_t)(nib | (other << 4));
    }
    if (__any(bad != ~0ull || ovf)) {
        for (int o = 32; o > 0; o >>= 1) {
            const uint64_t y = __shfl_xor(bad, o, 64);
            bad = y < bad ? y : bad;
            ovf |= __shfl_xor(ovf, o, 64);
        }
        if (lane == 0) {
            if (bad != ~0ull) atomicMin(a.res + AID_R_ERR_ROW, (unsigned long long)bad);
            if (ovf) atomicOr(a.res + AID_R_OVF, 1ull);
        }
    }
}

// ====================================================================== host side
#define TSQ_MAGIC_CAST 0x74737149u /* 'tsqI' */
// words of the context's 64-word pinned block this unit reads results back through (the entry points hold the context lock)
#define INS_PIN_ERR 32                    // the error word, then the five warning counts
#define INS_PIN_TOTAL (INS_PIN_ERR + 6)   // one total per table column (string columns)
#define AID_PIN_RES 32                    // tsq_autoid_fill's seven result words
static_assert(INS_PIN_TOTAL + TSQ_MAX_COLS <= 64 && AID_PIN_RES + 7 <= 64, "the context's pinned block holds 64 words");

struct tsq_cast {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    std::atomic<int> cancelled{0};
    int32_t n_cols = 0;
    uint32_t stmt_flags = 0;
    tsq_ins_col col[TSQ_MAX_COLS];
    DevBuf words;                                    // error word + warning counts
    DevBuf in_data[TSQ_MAX_COLS], in_null[TSQ_MAX_COLS], out_data[TSQ_MAX_COLS], out_null[TSQ_MAX_COLS];  // staging of host chunks
    DevBuf in_offs[TSQ_MAX_COLS], out_offs[TSQ_MAX_COLS];                                               // ... of their var-len columns
    DevBuf lens[TSQ_MAX_COLS], defs[TSQ_MAX_COLS], scan_tmp;  // string targets: cell lengths -> offsets; the defaults' bytes
    bool has_str = false, has_str_int = false;  // string targets; integer targets fed by a string column
    int64_t w_too_long = 0, w_bad_utf8 = 0, w_truncated = 0;
    uint32_t str_ctx = 0;
    uint64_t last_err = TSQ_INS_ERR_NONE;
    bool has_err = false;
    int64_t w_overflow = 0, w_bad_null = 0;
    int64_t rows = 0, launches = 0;
    double kernel_ms = 0;
    DevEvent ev[2];
};

TSQ_API tsq_status tsq_cast_create(tsq_ctx* ctx, const tsq_cast_col* cols, int32_t n_table_cols, uint32_t stmt_flags, uint32_t str_ctx, tsq_cast** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !out) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_cast_create: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (!cols || n_table_cols < 1) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_cast_create: no columns");
    if (n_table_cols > TSQ_MAX_COLS) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "tsq_cast_create: more than TSQ_MAX_COLS table columns");
    const uint32_t all_stmt = TSQ_CAST_IGNORE_TRUNCATE | TSQ_CAST_TRUNCATE_AS_WARNING | TSQ_CAST_OVERFLOW_AS_WARNING | TSQ_CAST_BAD_NULL_AS_WARNING |
                              TSQ_CAST_IN_INSERT | TSQ_CAST_SKIP_UTF8_CHECK;
    if ((stmt_flags & ~all_stmt) || (str_ctx & ~(uint32_t)TSQ_STRCTX_ALL)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_cast_create: unknown statement flag");
    std::unique_ptr<tsq_cast> c(new tsq_cast());
    c->hdr.magic = TSQ_MAGIC_CAST;
    c->ctx = ctx;
    c->n_cols = n_table_cols;
    c->stmt_flags = stmt_flags;
    c->str_ctx = str_ctx;
    for (int i = 0; i < n_table_cols; i++) {
        const char* why = "";
        if (cols[i].src_col < -1 || cols[i].src_col >= TSQ_MAX_COLS) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_cast_create: src_col out of range");
        const tsq_status st = tsq_ins_plan_col(cols[i], &c->col[i], &why);
        if (st != TSQ_OK) return tsq_fail(ch, st, "tsq_cast_create: column " + std::to_string(i) + ": " + why);
    }
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    tsq_status st = c->words.reserve(ctx, ch, 64);
    for (int i = 0; i < n_table_cols && st == TSQ_OK; i++) {
        if (c->col[i].kind != TSQ_INS_STR && c->col[i].src_col >= 0 && c->col[i].src_type == TSQ_BYTES) c->has_str_int = true;
        if (c->col[i].kind != TSQ_INS_STR) continue;
        c->has_str = true;
        st = c->defs[i].reserve(ctx, ch, (size_t)c->col[i].def_len + 64);
        if (st == TSQ_OK && c->col[i].def_len > 0 && hipMemcpy(c->defs[i].p, c->col[i].def_bytes, (size_t)c->col[i].def_len, hipMemcpyHostToDevice) != hipSuccess)
            st = tsq_fail(ch, TSQ_ERR_HIP, "tsq_cast_create: copying a default");
        c->col[i].def_bytes = nullptr;  // (the caller's pointer is not kept)
    }
    for (int i = 0; i < 2 && st == TSQ_OK; i++)
        if (c->ev[i].create() != hipSuccess) st = tsq_fail(ch, TSQ_ERR_HIP, "hipEventCreate");
    if (st != TSQ_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return st;
    }
    *out = c.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_cast_run(tsq_cast* c, const tsq_col* in_cols, int32_t n_in, int64_t nrows, tsq_col* out_cols, int64_t* cap_bytes, int64_t* bytes_out) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(c, TSQ_MAGIC_CAST));
    if (!c || c->hdr.magic != TSQ_MAGIC_CAST) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &c->hdr;
    c->has_err = false;
    c->w_overflow = c->w_bad_null = c->w_too_long = c->w_bad_utf8 = c->w_truncated = 0;
    if (c->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "cast cancelled");
    if (n_in < 0 || n_in > TSQ_MAX_COLS || nrows < 0 || !out_cols || (n_in > 0 && !in_cols)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: bad arguments");
    if (c->has_str && (!cap_bytes || !bytes_out)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: a table with a string column needs cap_bytes and bytes_out");
    if (nrows >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_cast_run: 2^31 rows or more");
    if (bytes_out)
        for (int i = 0; i < c->n_cols; i++) bytes_out[i] = 0;
    const bool dev = (out_cols[0].flags & TSQ_COL_DEVICE) != 0;
    for (int i = 0; i < c->n_cols; i++) {
        const tsq_ins_col& k = c->col[i];
        const bool str = k.kind == TSQ_INS_STR;
        if (((out_cols[i].flags & TSQ_COL_DEVICE) != 0) != dev) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: host and device columns mixed");
        if (out_cols[i].type != tsq_ins_out_type(k)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: out_cols[" + std::to_string(i) + "] has the wrong type");
        if (str && cap_bytes[i] < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: negative cap_bytes");
        if (nrows > 0 && !str && (!out_cols[i].data || !out_cols[i].null_bitmap)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: an output column lacks data or null_bitmap");
        if (nrows > 0 && str && cap_bytes[i] > 0 && (!out_cols[i].data || !out_cols[i].null_bitmap || !out_cols[i].offsets))
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: a string output column lacks data, offsets or null_bitmap");
        if (k.src_col >= 0) {
            if (k.src_col >= n_in) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: src_col beyond the input columns");
            const tsq_col& s = in_cols[k.src_col];
            if (s.type != k.src_type) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: in_cols[" + std::to_string(k.src_col) + "] has the wrong type");
            if (((s.flags & TSQ_COL_DEVICE) != 0) != dev) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: host and device columns mixed");
            if (s.length < nrows || (nrows > 0 && !s.data)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: an input column is shorter than nrows");
            if (s.type == TSQ_BYTES && nrows > 0 && !s.offsets) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: a string input column lacks offsets");
        }
    }
    if (nrows == 0) return TSQ_OK;
    tsq_ctx* ctx = c->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    InsCastArgs a;
    memset(&a, 0, sizeof a);
    a.n_cols = c->n_cols;
    a.stmt_flags = c->stmt_flags;
    a.str_ctx = c->str_ctx;
    a.nrows = nrows;
    a.bitmap_bytes = (int64_t)tsq_bitmap_bytes(nrows);
    a.err = c->words.as<unsigned long long>();
    a.warn = a.err + 1;
    // ---- inputs
    for (int i = 0; i < c->n_cols; i++) {
        const tsq_ins_col& k = c->col[i];
        a.col[i] = k;
        a.def_dev[i] = c->defs[i].as<uint8_t>();
        if (k.src_col < 0) continue;
        const tsq_col& s = in_cols[k.src_col];
        if (dev) {
            a.in_data[i] = s.data;
            a.in_null[i] = s.null_bitmap;
            a.in_offs[i] = s.offsets;
            continue;
        }
        size_t bytes = (size_t)nrows * (k.src_type == TSQ_F32 ? 4 : 8);
        const uint8_t* src = (const uint8_t*)s.data;
        if (k.src_type == TSQ_BYTES) {  // the cells' bytes [offsets[0], offsets[nrows]); the staged offsets keep indexing from the column's base
            if (s.offsets[nrows] < s.offsets[0] || s.offsets[0] < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: offsets of a string input column decrease");
            bytes = (size_t)s.offsets[nrows];
            TSQ_TRY(c->in_offs[i].reserve(ctx, h, ((size_t)nrows + 1) * 8 + 64));
            TSQ_HIP(h, hipMemcpyAsync(c->in_offs[i].p, s.offsets, ((size_t)nrows + 1) * 8, hipMemcpyHostToDevice, ctx->stream));
            a.in_offs[i] = c->in_offs[i].as<int64_t>();
        }
        TSQ_TRY(c->in_data[i].reserve(ctx, h, bytes + 64));
        if (bytes) TSQ_HIP(h, hipMemcpyAsync(c->in_data[i].p, src, bytes, hipMemcpyHostToDevice, ctx->stream));
        a.in_data[i] = c->in_data[i].p;
        if (s.null_bitmap) {
            TSQ_TRY(c->in_null[i].reserve(ctx, h, (size_t)a.bitmap_bytes + 64));
            TSQ_HIP(h, hipMemcpyAsync(c->in_null[i].p, s.null_bitmap, (size_t)a.bitmap_bytes, hipMemcpyHostToDevice, ctx->stream));
            a.in_null[i] = c->in_null[i].as<uint8_t>();
        }
    }
    TSQ_HIP(h, hipMemsetAsync(a.err, 0xff, 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(a.warn, 0, 40, ctx->stream));
    TSQ_HIP(h, hipEventRecord(c->ev[0], ctx->stream));
    const int sgrid = tsq_grid_for(ctx, nrows, 256);
    // ---- string columns: lengths -> offsets and sizes, before a byte of the caller's is written
    int64_t total[TSQ_MAX_COLS] = {0};
    if (c->has_str) {
        for (int i = 0; i < c->n_cols; i++)
            if (c->col[i].kind == TSQ_INS_STR) {
                TSQ_TRY(c->lens[i].reserve(ctx, h, ((size_t)nrows + 2) * 8 + 64));
                a.lens[i] = c->lens[i].as<int64_t>();
            }
        hipLaunchKernelGGL(k_ins_str<false>, dim3(sgrid), dim3(256), 0, ctx->stream, a);
        TSQ_HIP(h, hipGetLastError());
        c->launches += 1;
        for (int i = 0; i < c->n_cols; i++)
            if (c->col[i].kind == TSQ_INS_STR) {
                TSQ_TRY(tsq_launch_scan64(ctx, h, a.lens[i], nrows, c->scan_tmp));
                TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + INS_PIN_TOTAL + i, a.lens[i] + nrows, 8, hipMemcpyDeviceToHost, ctx->stream));
            }
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        bool small = false;
        for (int i = 0; i < c->n_cols; i++)
            if (c->col[i].kind == TSQ_INS_STR) {
                total[i] = (int64_t)ctx->pinned[INS_PIN_TOTAL + i];
                bytes_out[i] = total[i];
                small = small || total[i] > cap_bytes[i] || !out_cols[i].offsets || !out_cols[i].null_bitmap;
            }
        if (small) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_cast_run: output buffer too small (*bytes_out = bytes needed)");
    }
    // ---- outputs
    bool aligned = true;
    for (int i = 0; i < c->n_cols; i++) {
        const tsq_ins_col& k = c->col[i];
        const bool str = k.kind == TSQ_INS_STR;
        const size_t out_bytes = str ? (size_t)total[i] : (size_t)nrows * (k.out_f32 ? 4 : 8);
        if (dev) {
            a.out_data[i] = out_cols[i].data;
            a.out_null[i] = out_cols[i].null_bitmap;
            a.out_offs[i] = out_cols[i].offsets;
        } else {
            TSQ_TRY(c->out_data[i].reserve(ctx, h, out_bytes + 64));
            TSQ_TRY(c->out_null[i].reserve(ctx, h, (size_t)a.bitmap_bytes + 64));
            a.out_data[i] = c->out_data[i].p;
            a.out_null[i] = c->out_null[i].as<uint8_t>();
            if (str) {
                TSQ_TRY(c->out_offs[i].reserve(ctx, h, ((size_t)nrows + 1) * 8 + 64));
                a.out_offs[i] = c->out_offs[i].as<int64_t>();
            }
        }
        if (str) continue;
        if (k.src_col >= 0 && k.src_type != TSQ_BYTES) aligned = aligned && !((uintptr_t)a.in_data[i] & 15u);
        aligned = aligned && !((uintptr_t)a.out_data[i] & 15u) && !((uintptr_t)a.out_null[i] & 3u);
    }
    a.n_vec = aligned ? (nrows & ~(int64_t)127) : 0;
    hipLaunchKernelGGL(k_ins_cast_tpl<false>, dim3(tsq_grid_for(ctx, nrows, 256, 2)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    c->launches += 1;
    if (c->has_str_int) {
        hipLaunchKernelGGL(k_ins_cast_tpl<true>, dim3(sgrid), dim3(256), 0, ctx->stream, a);
        TSQ_HIP(h, hipGetLastError());
        c->launches += 1;
    }
    if (c->has_str) {
        hipLaunchKernelGGL(k_ins_str<true>, dim3(sgrid), dim3(256), 0, ctx->stream, a);
        TSQ_HIP(h, hipGetLastError());
        c->launches += 1;
    }
    TSQ_HIP(h, hipEventRecord(c->ev[1], ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + INS_PIN_ERR, a.err, 48, hipMemcpyDeviceToHost, ctx->stream));
    if (!dev) {
        for (int i = 0; i < c->n_cols; i++) {
            const bool str = c->col[i].kind == TSQ_INS_STR;
            const size_t out_bytes = str ? (size_t)total[i] : (size_t)nrows * (c->col[i].out_f32 ? 4 : 8);
            if (out_bytes) TSQ_HIP(h, hipMemcpyAsync(out_cols[i].data, a.out_data[i], out_bytes, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipMemcpyAsync(out_cols[i].null_bitmap, a.out_null[i], (size_t)a.bitmap_bytes, hipMemcpyDeviceToHost, ctx->stream));
            if (str) TSQ_HIP(h, hipMemcpyAsync(out_cols[i].offsets, a.out_offs[i], ((size_t)nrows + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
    }
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    c->rows += nrows;
    float ms = 0;
    if (hipEventElapsedTime(&ms, c->ev[0], c->ev[1]) == hipSuccess) c->kernel_ms += ms;
    const uint64_t errw = ctx->pinned[INS_PIN_ERR];
    if (errw != TSQ_INS_ERR_NONE) {
        c->has_err = true;
        c->last_err = errw;
        const tsq_status st = (tsq_status)tsq_ins_err_status(errw);
        const char* what = st == TSQ_ERR_OUT_OF_RANGE ? ": out of range value" : st == TSQ_ERR_BAD_NULL ? ": column cannot be null" : st == TSQ_ERR_DATA_TOO_LONG ? ": data too long"
                           : st == TSQ_ERR_BAD_UTF8 ? ": incorrect utf8 value" : st == TSQ_ERR_TRUNCATED_WRONG_VALUE ? ": truncated incorrect integer value"
                                                                                                                             : ": a NaN for an integer column";
        return tsq_fail(h, st, "cast: row " + std::to_string(tsq_ins_err_row(errw)) + ", column " + std::to_string(tsq_ins_err_col(errw)) + what);
    }
    c->w_overflow = (int64_t)ctx->pinned[INS_PIN_ERR + 1];
    c->w_bad_null = (int64_t)ctx->pinned[INS_PIN_ERR + 2];
    c->w_too_long = (int64_t)ctx->pinned[INS_PIN_ERR + 3];
    c->w_bad_utf8 = (int64_t)ctx->pinned[INS_PIN_ERR + 4];
    c->w_truncated = (int64_t)ctx->pinned[INS_PIN_ERR + 5];
    return TSQ_OK;
}

TSQ_API tsq_status tsq_cast_error_at(tsq_cast* c, int64_t* row, int32_t* table_col) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(c, TSQ_MAGIC_CAST));  // (tsq_cast_run writes what this reads)
    if (!c || c->hdr.magic != TSQ_MAGIC_CAST) return TSQ_ERR_INVALID;
    if (!c->has_err) return tsq_fail(&c->hdr, TSQ_ERR_INVALID, "tsq_cast_error_at: the last run returned no cell error");
    if (row) *row = tsq_ins_err_row(c->last_err);
    if (table_col) *table_col = tsq_ins_err_col(c->last_err);
    return TSQ_OK;
}

TSQ_API tsq_status tsq_cast_warnings(tsq_cast* c, int64_t* overflow, int64_t* truncated, int64_t* data_too_long, int64_t* bad_null, int64_t* bad_utf8) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(c, TSQ_MAGIC_CAST));  // (tsq_cast_run writes what this reads)
    if (!c || c->hdr.magic != TSQ_MAGIC_CAST) return TSQ_ERR_INVALID;
    if (overflow) *overflow = c->w_overflow;
    if (truncated) *truncated = c->w_truncated;
    if (data_too_long) *data_too_long = c->w_too_long;
    if (bad_null) *bad_null = c->w_bad_null;
    if (bad_utf8) *bad_utf8 = c->w_bad_utf8;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_cast_stats(tsq_cast* c, int64_t* rows, int64_t* launches, double* kernel_ms) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(c, TSQ_MAGIC_CAST));  // (tsq_cast_run writes what this reads)
    if (!c || c->hdr.magic != TSQ_MAGIC_CAST) return TSQ_ERR_INVALID;
    if (rows) *rows = c->rows;
    if (launches) *launches = c->launches;
    if (kernel_ms) *kernel_ms = c->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_cast_cancel(tsq_cast* c) {
    if (!c || c->hdr.magic != TSQ_MAGIC_CAST) return TSQ_ERR_INVALID;
    c->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_cast_destroy(tsq_cast* c) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(c, TSQ_MAGIC_CAST));
    if (!c || c->hdr.magic != TSQ_MAGIC_CAST) return;
    (void)hipSetDevice(c->ctx->device);
    (void)hipStreamSynchronize(c->ctx->stream);
    c->hdr.magic = 0;
    delete c;
}

TSQ_API tsq_status tsq_autoid_fill(tsq_ctx* ctx, tsq_col* col, int64_t nrows, int64_t base, uint32_t flags, int64_t upper_bound, int64_t* new_base,
                                   int64_t* first_allocated, int64_t* last_explicit, int64_t* error_row) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (new_base) *new_base = base;
    if (first_allocated) *first_allocated = 0;
    if (last_explicit) *last_explicit = 0;
    if (error_row) *error_row = -1;
    if (!col || !new_base || nrows < 0 || (flags & ~TSQ_AUTOID_NO_AUTO_VALUE_ON_ZERO) || (nrows > 0 && !col->data) || col->length < nrows)
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_autoid_fill: bad arguments");
    if (base < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_autoid_fill: a negative base (an allocator starts at 0 and never goes back)");
    if (col->type != TSQ_I64) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_autoid_fill: the auto-increment column must be a TSQ_I64 column");
    if (nrows >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_autoid_fill: 2^31 rows or more");
    if (nrows == 0) return TSQ_OK;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool dev = (col->flags & TSQ_COL_DEVICE) != 0;
    const size_t bm_bytes = tsq_bitmap_bytes(nrows);
    DevBuf data, nulls, work;
    StreamDrain drain(ctx->stream);  // every exit below waits for the stream: the kernels read the three buffers, the last copies write the caller's column
    auto hip_fail = [&](hipError_t e) { return tsq_fail(h, e == hipErrorOutOfMemory ? TSQ_ERR_OOM_DEVICE : TSQ_ERR_HIP, std::string("tsq_autoid_fill: ") + hipGetErrorString(e)); };
    AidArgs a;
    memset(&a, 0, sizeof a);
    a.n = nrows;
    a.base = base;
    a.upper = upper_bound;
    a.flags = flags;
    a.n_tiles = (nrows + TSQ_AID_TILE - 1) / TSQ_AID_TILE;
    tsq_status st = TSQ_OK;
    hipError_t e = hipSuccess;
    if (dev) {
        a.data = (int64_t*)col->data;
        a.nulls = col->null_bitmap;
    } else {
        st = data.reserve(ctx, h, (size_t)nrows * 8 + 64);
        if (st == TSQ_OK && col->null_bitmap) st = nulls.reserve(ctx, h, bm_bytes + 64);
        TSQ_TRY(st);
        e = hipMemcpyAsync(data.p, col->data, (size_t)nrows * 8, hipMemcpyHostToDevice, ctx->stream);
        if (e == hipSuccess && col->null_bitmap) e = hipMemcpyAsync(nulls.p, col->null_bitmap, bm_bytes, hipMemcpyHostToDevice, ctx->stream);
        if (e != hipSuccess) return hip_fail(e);
        a.data = data.as<int64_t>();
        a.nulls = col->null_bitmap ? nulls.as<uint8_t>() : nullptr;
    }
    a.vec = ((uintptr_t)a.data & 15u) ? 0 : 1;
    // work: agg | tile_first | tile_last | s_in | res
    const size_t nt = (size_t)a.n_tiles;
    const size_t agg_bytes = (nt * sizeof(tsq_aid_op) + 63) & ~(size_t)63, w8 = (nt * 8 + 63) & ~(size_t)63;
    TSQ_TRY(work.reserve(ctx, h, agg_bytes + 3 * w8 + 64));
    char* wp = work.as<char>();
    a.agg = (tsq_aid_op*)wp;
    a.tile_first = (int64_t*)(wp + agg_bytes);
    a.tile_last = (int64_t*)(wp + agg_bytes + w8);
    a.s_in = (int64_t*)(wp + agg_bytes + 2 * w8);
    a.res = (unsigned long long*)(wp + agg_bytes + 3 * w8);
    e = hipMemsetAsync(a.res, 0, 64, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.res + AID_R_ERR_ROW, 0xff, 8, ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    hipLaunchKernelGGL(k_aid_agg, dim3((unsigned)a.n_tiles), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_aid_scan, dim3(1), dim3(1024), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_aid_apply, dim3((unsigned)a.n_tiles), dim3(256), 0, ctx->stream, a);
    e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned + AID_PIN_RES, a.res, 56, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    const uint64_t* r = ctx->pinned + AID_PIN_RES;
    if (r[AID_R_ERR_ROW] != ~0ull) {
        if (error_row) *error_row = (int64_t)r[AID_R_ERR_ROW];
        return tsq_fail(h, TSQ_ERR_OUT_OF_RANGE, "auto-increment id out of range at row " + std::to_string((int64_t)r[AID_R_ERR_ROW]));
    }
    if (r[AID_R_OVF]) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_autoid_fill: the allocator passes INT64_MAX");
    if (!dev) {
        e = hipMemcpyAsync(col->data, a.data, (size_t)nrows * 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess && col->null_bitmap) e = hipMemcpyAsync(col->null_bitmap, a.nulls, bm_bytes, hipMemcpyDeviceToHost, ctx->stream);
        if (e != hipSuccess) return hip_fail(e);
    }
    *new_base = (int64_t)r[AID_R_NEW_BASE];
    if (first_allocated && (int64_t)r[AID_R_FIRST_ROW] != TSQ_I64MAX) *first_allocated = (int64_t)r[AID_R_FIRST_VAL];
    if (last_explicit && (int64_t)r[AID_R_LAST_ROW] >= 0) *last_explicit = (int64_t)r[AID_R_LAST_VAL];
    return TSQ_OK;
}
