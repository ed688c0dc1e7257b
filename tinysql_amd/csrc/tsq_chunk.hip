// tsq_chunk.hip — chunk-level data movement between GPU operators (gfx950).
//
// tsq_chunk_compact replaces what the reference does when an operator hands a FILTERED chunk on: SelectionExec copies the
// selected rows into the output chunk (executor/executor.go:393-438) / Column.CopyReconstruct gathers by the selection
// vector (util/chunk/column.go:504-552).  With device-resident chunks this is the hand-off between a GPU Selection and a
// GPU join / aggregate: no D2H, the dense chunk never leaves HBM.
//   K12a k_compact_count  : selected rows per WAVE (every wave owns a contiguous run of rows)
//   K12b k_compact_scatter: exclusive bases by k_compact_scan (one workgroup) -> a running cursor per wave in a register, wave
//                           ballot + popcount prefix, every column's cell copied to its dense position; NULL flags as bytes ->
//                           k_pack_bitmap
// Algorithmic bytes: 1 B flag + (8 B read + 8 B written per SELECTED cell).  ROW ORDER IS PRESERVED: a wave walks its rows in
// order and the waves' output ranges follow each other — what SelectionExec / CopyReconstruct guarantee (a Limit above a
// Selection, a keep-order table scan: store/mockstore/mocktikv/executor.go:360-390, :472-507).  (The first version handed out
// positions from one LDS cursor per workgroup: the four waves raced for it and the output was the input order only up to a
// permutation inside 256-row tiles.)
#include "tsq_stage.h"
#include "tsq_compact.h"

__global__ void __launch_bounds__(256) k_compact_scatter(CompactArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = u * a.rows_per_wave;  // a multiple of 64
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.nrows ? hi : a.nrows;
    unsigned long long cur = a.block_base[u];  // first output row of this wave's run (wave uniform)
    for (int64_t r = lo + lane; r - lane < hi; r += 64) {
        const bool sel = r < hi && a.selected[r];
        const unsigned long long m = __ballot(sel);
        const unsigned long long pos = cur + __popcll(m & ((1ull << lane) - 1ull));
        cur += (unsigned long long)__popcll(m);
        if (!sel) continue;
        if (a.src_row) a.src_row[pos] = (uint32_t)r;
        for (int c = 0; c < a.in.n; c++) {
            if (a.in.type[c] == TSQ_BYTES) a.out_offs[c][pos] = a.in.offs[c][r + 1] - a.in.offs[c][r];
            else if (a.in.type[c] == TSQ_F32) ((uint32_t*)a.out_data[c])[pos] = ((const uint32_t*)a.in.data[c])[r];
            else ((uint64_t*)a.out_data[c])[pos] = ((const uint64_t*)a.in.data[c])[r];
            if (a.out_notnull[c]) a.out_notnull[c][pos] = tsq_is_null(a.in.nulls[c], r) ? 0 : 1;
        }
    }
}
// the bytes of the selected cells of one var-len column (Column.CopyReconstruct of a var-len column, column.go:504-552): one cell per
// lane for short cells, one per wave (64 lanes on consecutive bytes) for long ones
template <bool WAVE>
__global__ void __launch_bounds__(256) k_compact_varlen(const uint8_t* src, const int64_t* src_offs, const uint32_t* src_row, const int64_t* out_offs,
                                                        uint8_t* dst, int64_t n_out) {
    const int lane = threadIdx.x & 63;
    const int64_t me = WAVE ? ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6 : (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    const int64_t step = WAVE ? ((int64_t)gridDim.x * blockDim.x) >> 6 : (int64_t)gridDim.x * blockDim.x;
    for (int64_t p = me; p < n_out; p += step) {
        const uint8_t* s = src + src_offs[src_row[p]];
        uint8_t* d = dst + out_offs[p];
        const int64_t n = out_offs[p + 1] - out_offs[p];
        if (WAVE) {
            for (int64_t i = lane; i < n; i += 64) d[i] = s[i];
        } else {
            tsq_copy_cell(d, s, n);
        }
    }
}

TSQ_API tsq_status tsq_chunk_compact(tsq_ctx* ctx, const tsq_col* cols, int32_t n_cols, int64_t nrows, const uint8_t* selected,
                                     tsq_col* out_cols, int64_t* nrows_out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (!cols || !out_cols || !nrows_out || !selected || n_cols < 1 || n_cols > TSQ_MAX_COLS || nrows < 0)
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_compact: bad arguments");
    *nrows_out = 0;
    for (int c = 0; c < n_cols; c++) {
        if (!(cols[c].flags & TSQ_COL_DEVICE) || !(out_cols[c].flags & TSQ_COL_DEVICE))
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_compact: columns (and the selected[] flags) must be device resident");
        if (cols[c].type < TSQ_I64 || cols[c].type > TSQ_BYTES) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_compact: unknown column type");
        if (cols[c].null_bitmap && !out_cols[c].null_bitmap) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_compact: nullable column needs an output bitmap");
        if (cols[c].type == TSQ_BYTES) {
            // a var-len output column needs offsets[nrows + 1] and a data array as large as the input's (a selection never grows)
            if (nrows > 0 && (!cols[c].offsets || !out_cols[c].offsets)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_compact: var-len column needs offsets on both sides");
            if (nrows >= 0xffffffffLL) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_chunk_compact: var-len chunk beyond 2^32 rows");
        } else if (nrows > 0 && (!cols[c].data || !out_cols[c].data)) {
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_compact: NULL data pointer");
        }
    }
    if (nrows == 0) {
        for (int c = 0; c < n_cols; c++)
            if (cols[c].type == TSQ_BYTES && out_cols[c].offsets) TSQ_HIP(h, hipMemsetAsync(out_cols[c].offsets, 0, 8, ctx->stream));
        return TSQ_OK;
    }
    TSQ_HIP(h, hipSetDevice(ctx->device));
    CompactArgs a;
    memset(&a, 0, sizeof a);
    tsq_colset_from_cols(a.in, cols, n_cols);
    a.selected = selected;
    a.nrows = nrows;
    const int grid = tsq_grid_for(ctx, nrows, 256);
    const int n_runs = grid * 4;
    a.rows_per_wave = (((nrows + n_runs - 1) / n_runs) + 63) & ~(int64_t)63;
    DevBuf base, srow, scratch;
    std::vector<DevBuf> nn(n_cols);
    tsq_status s = base.reserve(ctx, h, (size_t)n_runs * 8 + 64);
    bool any_var = false;
    for (int c = 0; c < n_cols; c++) any_var = any_var || cols[c].type == TSQ_BYTES;
    if (s == TSQ_OK && any_var) {
        s = srow.reserve(ctx, h, (size_t)nrows * 4 + 64);
        a.src_row = srow.as<uint32_t>();
    }
    for (int c = 0; c < n_cols && s == TSQ_OK; c++) {
        a.out_data[c] = out_cols[c].data;
        a.out_offs[c] = cols[c].type == TSQ_BYTES ? out_cols[c].offsets : nullptr;
        if (cols[c].null_bitmap) {
            s = nn[c].reserve(ctx, h, (size_t)nrows + 64);
            a.out_notnull[c] = nn[c].as<uint8_t>();
        }
    }
    TSQ_TRY(s);
    a.block_base = base.as<unsigned long long>();
    a.total = a.block_base + n_runs;
    hipLaunchKernelGGL(k_compact_count, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, a.block_base, n_runs, a.total);
    hipLaunchKernelGGL(k_compact_scatter, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipError_t e = hipGetLastError();
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned + 16, a.total, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_chunk_compact: ") + hipGetErrorString(e));
    const int64_t n_out = (int64_t)ctx->pinned[16];
    for (int c = 0; c < n_cols && s == TSQ_OK; c++) {
        if (a.out_notnull[c]) s = tsq_launch_pack_bitmap(ctx, h, a.out_notnull[c], out_cols[c].null_bitmap, n_out);
        else if (out_cols[c].null_bitmap && n_out > 0) {
            e = hipMemsetAsync(out_cols[c].null_bitmap, 0xff, tsq_bitmap_bytes(n_out), ctx->stream);
            if (e != hipSuccess) s = tsq_fail(h, TSQ_ERR_HIP, hipGetErrorString(e));
        }
        out_cols[c].length = n_out;
        out_cols[c].type = cols[c].type;
        out_cols[c].elem_size = cols[c].type == TSQ_BYTES ? -1 : tsq_elem_size(cols[c].type);
        if (cols[c].type == TSQ_BYTES && s == TSQ_OK) {  // lengths -> offsets, then the bytes
            s = tsq_launch_scan64(ctx, h, out_cols[c].offsets, n_out, scratch);
            if (s == TSQ_OK && n_out > 0) {
                e = hipMemcpyAsync(ctx->pinned + 17, out_cols[c].offsets + n_out, 8, hipMemcpyDeviceToHost, ctx->stream);
                if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
                if (e != hipSuccess) s = tsq_fail(h, TSQ_ERR_HIP, hipGetErrorString(e));
                const int64_t nbytes = (int64_t)ctx->pinned[17];
                if (s == TSQ_OK && nbytes > 0) {
                    if (nbytes / n_out > 32)
                        hipLaunchKernelGGL(k_compact_varlen<true>, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, (const uint8_t*)cols[c].data, cols[c].offsets,
                                           a.src_row, out_cols[c].offsets, (uint8_t*)out_cols[c].data, n_out);
                    else
                        hipLaunchKernelGGL(k_compact_varlen<false>, dim3(tsq_grid_for(ctx, n_out, 256)), dim3(256), 0, ctx->stream, (const uint8_t*)cols[c].data,
                                           cols[c].offsets, a.src_row, out_cols[c].offsets, (uint8_t*)out_cols[c].data, n_out);
                    e = hipGetLastError();
                    if (e != hipSuccess) s = tsq_fail(h, TSQ_ERR_HIP, hipGetErrorString(e));
                }
            }
        }
    }
    if (s == TSQ_OK) {
        e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) s = tsq_fail(h, TSQ_ERR_HIP, hipGetErrorString(e));
    }
    TSQ_TRY(s);
    *nrows_out = n_out;
    return TSQ_OK;
}

// ---------------------------------------------------------------- device-side append of a chunk to a chunk
// What chunk.Chunk.Append does for the reference's operators that collect their child's rows (util/chunk/chunk.go:302-332), between two
// device chunks: fixed-width cells and string bytes by device copies, the null bitmap through k_append_bits at any bit offset, the
// offsets of a string column moved behind the bytes the destination already holds (k_offsets_rebase).  Nothing is read on the host but the
// three offsets that size a string column's copy.
//   K12c k_bytes_or : dst[i] |= src[i] — two flag arrays (one byte per row) into one
__global__ void __launch_bounds__(256) k_bytes_or(uint8_t* dst, const uint8_t* src, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * 256 + threadIdx.x; i < n; i += (int64_t)gridDim.x * 256) dst[i] = dst[i] | src[i];
}

TSQ_API tsq_status tsq_bytes_or(tsq_ctx* ctx, uint8_t* dst, const uint8_t* src, int64_t n) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (n < 0 || (n > 0 && (!dst || !src))) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_bytes_or: bad arguments");
    if (n == 0) return TSQ_OK;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_bytes_or, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, dst, src, n);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_chunk_append(tsq_ctx* ctx, const tsq_col* dst_cols, int64_t dst_rows, const int64_t* dst_cap_bytes, const tsq_col* src_cols, int32_t n_cols,
                                    int64_t n) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (n < 0 || dst_rows < 0 || n_cols < 0 || (n_cols > 0 && (!dst_cols || !src_cols))) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: bad arguments");
    if (dst_rows + n >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_chunk_append: 2^31 rows or more");
    for (int c = 0; c < n_cols; c++) {
        const tsq_col &d = dst_cols[c], &s = src_cols[c];
        if (d.type != s.type || !(d.flags & TSQ_COL_DEVICE) || !(s.flags & TSQ_COL_DEVICE))
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: columns must be device resident and of the same types");
        if (d.length < dst_rows + n || s.length < n) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: the destination has no room for the rows");
        if (s.null_bitmap && !d.null_bitmap) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: a nullable source needs a destination bitmap");
        if (d.type == TSQ_BYTES && (!d.offsets || !s.offsets || !dst_cap_bytes)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: a string column without offsets");
        if (n > 0 && ((!d.data && d.type != TSQ_BYTES) || (!s.data && s.type != TSQ_BYTES))) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: a column without data");
    }
    if (n == 0) return TSQ_OK;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    for (int c = 0; c < n_cols; c++) {
        const tsq_col &d = dst_cols[c], &s = src_cols[c];
        if (d.null_bitmap) TSQ_TRY(tsq_launch_append_bits(ctx, h, d.null_bitmap, dst_rows, s.null_bitmap, n));  // (no source bitmap: n set bits)
        if (d.type != TSQ_BYTES) {
            const size_t es = (size_t)tsq_elem_size(d.type);
            TSQ_HIP(h, hipMemcpyAsync((char*)d.data + (size_t)dst_rows * es, s.data, (size_t)n * es, hipMemcpyDeviceToDevice, ctx->stream));
            continue;
        }
        ctx->pinned[58] = 0;
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 56, s.offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 57, s.offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        if (dst_rows > 0) TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 58, d.offsets + dst_rows, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        const int64_t lo = (int64_t)ctx->pinned[56], hi = (int64_t)ctx->pinned[57], base = (int64_t)ctx->pinned[58];
        if (lo < 0 || hi < lo || base < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: string offsets decrease");
        if (base + (hi - lo) > dst_cap_bytes[c]) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_chunk_append: the destination's string bytes have no room");
        if (hi > lo) TSQ_HIP(h, hipMemcpyAsync((char*)d.data + base, (const char*)s.data + lo, (size_t)(hi - lo), hipMemcpyDeviceToDevice, ctx->stream));
        TSQ_TRY(tsq_launch_offsets_rebase(ctx, h, d.offsets + dst_rows, s.offsets, n + 1, base - lo));
    }
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}
