// tsq_memread.hip — the mem readers' view of the transaction buffer on the GPU (gfx950): iterTxnMemBuffer (executor/mem_reader.go:256-281)
// over the arrays the last tsq_membuf_finish left, the point reads of memIndexLookUpReader.getMemRows (:359-398) and the dirty handles
// of a table (executor/union_scan.go DirtyTable :56-74) — include/tsq.h "Transaction buffer: mem readers"; DESIGN.md §5 "Mem readers".
// The per-position code is tsq_memread_dp.h.
//
// tsq_membuf_scan / tsq_membuf_scan_points:
//   K26a k_mr_bounds   : one lane per range bound (2 per range: neighbouring lanes, the even one takes the odd one's answer by a
//                        shuffle) or per point key — the lower-bound search over the finished keys; first entry and entry count per range
//        tsq_launch_scan64 over the counts -> the first position of every range  (the host reads the position total and the error bits)
//   K26b k_mr_mark     : one lane per position — position -> range by binary search over that scan, range -> entry, keep = (op == PUT),
//                        the pair's key and value lengths; the skipped deletes are counted
//        tsq_launch_scan64 x 3: the pair ordinal and the two byte offsets of every position
//   K26c k_mr_rcounts  : one lane per range — its pairs, from the ordinals at its two ends (only when the caller asks for them)
//        (the host reads the totals: second and last synchronisation)
// tsq_membuf_fetch:
//   K26d k_mr_copy     : one lane per position — the kept pairs' offsets, keys and values at their place; a cell of the threshold length
//                        (TSQ_KNOB_ROWENC_WAVE_COPY, 64) or more is copied by the whole wave, as k_mb_copy does; desc places pair o at
//                        n_pairs - 1 - o and its bytes at total - begin - length: the suffix form of the same scan
// tsq_membuf_dirty / tsq_membuf_dirty_fetch:
//        k_mr_bounds over the table's record range, then
//   K26e k_mr_dirty_mark  : one lane per entry of the range — its handle, and a flag in the added (PUT) or deleted (DEL) list
//        tsq_launch_scan64 x 2
//   K26f k_mr_dirty_write : the handles at their place in either list; both fall out ascending, the keys are
// Every kernel is a grid-stride loop sized by a count the host knows; no kernel assumes n > 0.
#include "tsq_membuf_store.h"
#include "tsq_memread_dp.h"

#define TSQ_MR_DEFAULT_WAVE_COPY 64

// the words the kernels of one call share and the host reads
struct MrCtl {
    unsigned int err;
    unsigned int pad;
    unsigned long long dels;
};

struct MrBoundArgs {
    tsq_mr_buffer b;
    const uint8_t* bytes;  // the range bytes, or the point keys
    const int64_t* offs;   // ranges: [2 n + 1]; points: [n + 1] or NULL
    int64_t fixed_len, key_bytes;
    int64_t n;             // ranges or points
    int32_t points;
    int64_t* rlo;          // [n]
    int64_t* rcnt;         // [n + 1]: the entries of every range; then (scan) its first position
    MrCtl* ctl;
};
__global__ void __launch_bounds__(256) k_mr_bounds(MrBoundArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    const int64_t nb = a.points ? a.n : 2 * a.n;
    uint32_t err = 0;
    for (int64_t j0 = wave * 64; j0 < nb; j0 += nwaves * 64) {  // (wave uniform; j0 is even, so a range's two bounds share a wave)
        const int64_t j = j0 + lane;
        int64_t pos = 0, cnt = 0;
        if (j < nb) pos = a.points ? tsq_mr_point(a.b, a.bytes, a.offs, a.fixed_len, a.key_bytes, j, &cnt, &err) : tsq_mr_range_bound(a.b, a.bytes, a.offs, j, &err);
        const int64_t other = (int64_t)__shfl_xor((unsigned long long)pos, 1, 64);
        if (j < nb) {
            if (a.points) {
                a.rlo[j] = pos;
                a.rcnt[j] = cnt;
            } else if (!(j & 1)) {
                a.rlo[j >> 1] = pos;
                a.rcnt[j >> 1] = tsq_mr_range_count(pos, other);
            }
        }
    }
    if (err) atomicOr(&a.ctl->err, err);
}

struct MrMarkArgs {
    tsq_mr_buffer b;
    const int64_t* rlo;
    const int64_t* rbase;  // [n_ranges + 1]
    int64_t n_ranges;
    int64_t positions;
    int32_t* entry;  // [positions]
    int64_t* ord;    // [positions + 1] each: the flag and the lengths; then (scan) the ordinal and the offsets
    int64_t* koff;
    int64_t* voff;
    int64_t* rc;     // k_mr_rcounts: [n_ranges]
    MrCtl* ctl;
};
__global__ void __launch_bounds__(256) k_mr_mark(MrMarkArgs a) {
    unsigned long long dels = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.positions; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t e, kl, vl;
        bool del;
        const bool keep = tsq_mr_mark(a.b, a.rlo, a.rbase, a.n_ranges, p, &e, &del, &kl, &vl);
        a.entry[p] = (int32_t)e;  // (e < m < 2^31)
        a.ord[p] = keep ? 1 : 0;
        a.koff[p] = kl;
        a.voff[p] = vl;
        dels += del ? 1ull : 0ull;
    }
    for (int o = 32; o > 0; o >>= 1) dels += __shfl_xor(dels, o, 64);
    if ((threadIdx.x & 63) == 0 && dels) atomicAdd(&a.ctl->dels, dels);
}
__global__ void __launch_bounds__(256) k_mr_rcounts(MrMarkArgs a) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.n_ranges; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t lo = a.rbase[r], hi = a.rbase[r + 1];
        lo = lo < 0 ? 0 : (lo > a.positions ? a.positions : lo);  // (a scan of counts stays inside their sum: checked, not assumed)
        hi = hi < lo ? lo : (hi > a.positions ? a.positions : hi);
        a.rc[r] = a.ord[hi] - a.ord[lo];
    }
}

struct MrCopyArgs {
    tsq_mr_buffer b;
    const uint8_t* ovals;
    int64_t okey_bytes, oval_bytes;
    const int32_t* entry;
    const int64_t* ord;
    const int64_t* koff;
    const int64_t* voff;
    int64_t positions, n_pairs, key_bytes, value_bytes;
    int32_t desc;
    int64_t wave_copy;
    uint8_t* keys;
    int64_t* key_offsets;
    uint8_t* values;
    int64_t* value_offsets;
};
// every lane of the wave brings one cell (len 0: none): short cells by their lane, long ones by the whole wave, one after the other
__device__ __forceinline__ void mr_copy_cells(int lane, const uint8_t* s, uint8_t* d, int64_t len, int64_t wave_copy) {
    const bool by_wave = wave_copy > 0 && len >= wave_copy;
    if (len > 0 && !by_wave) tsq_copy_cell(d, s, len);
    unsigned long long todo = __ballot(by_wave);
    while (todo) {  // (wave uniform)
        const int src_lane = __ffsll((long long)todo) - 1;
        todo &= todo - 1;
        const uint8_t* ws = (const uint8_t*)__shfl((unsigned long long)s, src_lane, 64);
        uint8_t* wd = (uint8_t*)__shfl((unsigned long long)d, src_lane, 64);
        const int64_t wn = (int64_t)__shfl((unsigned long long)len, src_lane, 64);
        for (int64_t i = lane; i < wn; i += 64) wd[i] = ws[i];
    }
}
__global__ void __launch_bounds__(256) k_mr_copy(MrCopyArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.key_offsets[a.n_pairs] = a.key_bytes;
        a.value_offsets[a.n_pairs] = a.value_bytes;
    }
    for (int64_t p0 = wave * 64; p0 < a.positions; p0 += nwaves * 64) {  // (wave uniform)
        const int64_t p = p0 + lane;
        int64_t kl = 0, vl = 0;
        const uint8_t* ks = a.b.okeys;
        const uint8_t* vs = a.ovals;
        uint8_t* kd = a.keys;
        uint8_t* vd = a.values;
        if (p < a.positions && a.ord[p + 1] != a.ord[p]) {
            const int64_t e = a.entry[p], at = tsq_mr_place(a.ord[p], a.n_pairs, a.desc);
            if (e >= 0 && e < a.b.m && at >= 0 && at < a.n_pairs) {
                const int64_t sk = a.b.okoff[e], sv = a.b.ovoff[e];
                const int64_t l0 = a.koff[p + 1] - a.koff[p], l1 = a.voff[p + 1] - a.voff[p];
                const int64_t dk = tsq_mr_place_bytes(a.koff[p], l0, a.key_bytes, a.desc), dv = tsq_mr_place_bytes(a.voff[p], l1, a.value_bytes, a.desc);
                if (l0 >= 0 && l1 >= 0 && sk >= 0 && sk + l0 <= a.okey_bytes && sv >= 0 && sv + l1 <= a.oval_bytes && dk >= 0 && dk + l0 <= a.key_bytes && dv >= 0 &&
                    dv + l1 <= a.value_bytes) {
                    a.key_offsets[at] = dk;
                    a.value_offsets[at] = dv;
                    kl = l0, vl = l1;
                    ks += sk, vs += sv, kd += dk, vd += dv;
                }
            }
        }
        mr_copy_cells(lane, ks, kd, kl, a.wave_copy);
        mr_copy_cells(lane, vs, vd, vl, a.wave_copy);
    }
}

struct MrDirtyArgs {
    tsq_mr_buffer b;
    int64_t lo, positions;  // the entries [lo, lo + positions) of the table's record range
    int64_t* handle;        // [positions]
    int64_t* added;         // [positions + 1] each: the flag; then (scan) the place
    int64_t* deleted;
    int64_t n_added, n_deleted;
    int64_t* added_out;
    int64_t* deleted_out;
    MrCtl* ctl;
};
__global__ void __launch_bounds__(256) k_mr_dirty_mark(MrDirtyArgs a) {
    uint32_t err = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.positions; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t e = a.lo + p;
        int64_t h = 0;
        uint8_t op = TSQ_MVCC_OP_LOCK;
        if (e >= 0 && e < a.b.m) op = tsq_mr_dirty_at(a.b, e, &h, &err);
        a.handle[p] = h;
        a.added[p] = op == TSQ_MVCC_OP_PUT ? 1 : 0;
        a.deleted[p] = op == TSQ_MVCC_OP_DEL ? 1 : 0;
    }
    if (err) atomicOr(&a.ctl->err, err);
}
__global__ void __launch_bounds__(256) k_mr_dirty_write(MrDirtyArgs a) {
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.positions; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t ia = a.added[p], id = a.deleted[p];
        if (a.added[p + 1] != ia && ia >= 0 && ia < a.n_added) a.added_out[ia] = a.handle[p];
        if (a.deleted[p + 1] != id && id >= 0 && id < a.n_deleted) a.deleted_out[id] = a.handle[p];
    }
}

// ====================================================================== host side
namespace {
void mr_buffer_view(const tsq_membuf* mb, tsq_mr_buffer* b) {
    b->okeys = mb->okeys.as<uint8_t>();
    b->okoff = mb->okoff.as<int64_t>();
    b->oops = mb->oops.as<uint8_t>();
    b->ovoff = mb->ovoff.as<int64_t>();
    b->m = mb->m;
}

// the caller's array on the device: its own, or a copy in `own`
tsq_status mr_dev_array(tsq_membuf* mb, DevBuf& own, const void* src, size_t bytes, bool dev, const void** out) {
    *out = src;
    if (dev || !src || !bytes) return TSQ_OK;
    TSQ_TRY(own.reserve(mb->ctx, &mb->hdr, bytes + 64));
    TSQ_HIP(&mb->hdr, hipMemcpyAsync(own.p, src, bytes, hipMemcpyHostToDevice, mb->ctx->stream));
    *out = own.p;
    return TSQ_OK;
}

// bounds -> positions -> marks -> ordinals and offsets; what tsq_membuf_fetch needs stays in the handle
tsq_status mr_scan(tsq_membuf* mb, MrBoundArgs& a, int32_t desc, tsq_membuf_scan_result* result, int64_t* range_counts) {
    tsq_handle_hdr* h = &mb->hdr;
    tsq_ctx* ctx = mb->ctx;
    const int64_t n = a.n;
    mb->mr_have = false;
    if (n > 0) {
        TSQ_TRY(mb->mr_rlo.reserve(ctx, h, (size_t)n * 8 + 64));
        TSQ_TRY(mb->mr_rbase.reserve(ctx, h, ((size_t)n + 1) * 8 + 64));
    }
    TSQ_TRY(mb->mr_ctl.reserve(ctx, h, sizeof(MrCtl) + 64));
    TSQ_HIP(h, hipMemsetAsync(mb->mr_ctl.p, 0, sizeof(MrCtl), ctx->stream));
    mr_buffer_view(mb, &a.b);
    a.rlo = mb->mr_rlo.as<int64_t>();
    a.rcnt = mb->mr_rbase.as<int64_t>();
    a.ctl = mb->mr_ctl.as<MrCtl>();
    int64_t positions = 0;
    MrCtl ctl;
    memset(&ctl, 0, sizeof ctl);
    if (n > 0) {
        hipLaunchKernelGGL(k_mr_bounds, dim3(tsq_grid_for(ctx, a.points ? n : 2 * n, 256)), dim3(256), 0, ctx->stream, a);
        TSQ_HIP(h, hipGetLastError());
        TSQ_TRY(tsq_launch_scan64(ctx, h, a.rcnt, n, mb->mr_tmp));
        TSQ_HIP(h, hipMemcpyAsync(&positions, a.rcnt + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(&ctl, mb->mr_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // the position total sizes the per-position buffers
        if (ctl.err) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: offsets decrease or leave their buffer");
        if (positions < 0) return tsq_fail(h, TSQ_ERR_HIP, "internal: the position count of a buffer scan is out of range");
        if (positions >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "membuf: 2^31 scan positions or more");
    }
    int64_t tot[3] = {0, 0, 0};
    if (range_counts)
        for (int64_t r = 0; r < n; r++) range_counts[r] = 0;
    if (positions > 0) {
        TSQ_TRY(mb->mr_entry.reserve(ctx, h, (size_t)positions * 4 + 64));
        for (DevBuf* b : {&mb->mr_ord, &mb->mr_koff, &mb->mr_voff}) TSQ_TRY(b->reserve(ctx, h, ((size_t)positions + 1) * 8 + 64));
        MrMarkArgs k;
        memset(&k, 0, sizeof k);
        k.b = a.b, k.rlo = a.rlo, k.rbase = a.rcnt, k.n_ranges = n, k.positions = positions;
        k.entry = mb->mr_entry.as<int32_t>(), k.ord = mb->mr_ord.as<int64_t>(), k.koff = mb->mr_koff.as<int64_t>(), k.voff = mb->mr_voff.as<int64_t>();
        k.ctl = a.ctl;
        hipLaunchKernelGGL(k_mr_mark, dim3(tsq_grid_for(ctx, positions, 256)), dim3(256), 0, ctx->stream, k);
        TSQ_HIP(h, hipGetLastError());
        TSQ_TRY(tsq_launch_scan64(ctx, h, k.ord, positions, mb->mr_tmp));
        TSQ_TRY(tsq_launch_scan64(ctx, h, k.koff, positions, mb->mr_tmp));
        TSQ_TRY(tsq_launch_scan64(ctx, h, k.voff, positions, mb->mr_tmp));
        if (range_counts) {
            TSQ_TRY(mb->mr_rc.reserve(ctx, h, (size_t)n * 8 + 64));
            k.rc = mb->mr_rc.as<int64_t>();
            hipLaunchKernelGGL(k_mr_rcounts, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, k);
            TSQ_HIP(h, hipGetLastError());
            TSQ_HIP(h, hipMemcpyAsync(range_counts, k.rc, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        }
        TSQ_HIP(h, hipMemcpyAsync(&tot[0], k.ord + positions, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(&tot[1], k.koff + positions, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(&tot[2], k.voff + positions, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(&ctl, mb->mr_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // the counts and the status
        if (tot[0] < 0 || tot[0] > positions || tot[1] < 0 || tot[2] < 0 || (int64_t)ctl.dels < 0 || tot[0] + (int64_t)ctl.dels > positions)
            return tsq_fail(h, TSQ_ERR_HIP, "internal: the pair counts of a buffer scan are out of range");
    }
    mb->mr_have = true;
    mb->mr_desc = desc ? 1 : 0;
    mb->mr_positions = positions;
    mb->mr_pairs = tot[0];
    mb->mr_key_bytes = tot[1];
    mb->mr_value_bytes = tot[2];
    result->n_pairs = tot[0];
    result->key_bytes = tot[1];
    result->value_bytes = tot[2];
    result->positions = positions;
    result->skipped_dels = (int64_t)ctl.dels;
    return TSQ_OK;
}

tsq_status mr_enter(tsq_membuf* mb, void* result, size_t result_bytes) {
    tsq_handle_hdr* h = &mb->hdr;
    if (!result) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL result");
    memset(result, 0, result_bytes);
    mb->mr_have = false;  // whatever becomes of this scan, the last one can no longer be fetched
    if (!mb->finished) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: not finished");
    TSQ_HIP(h, hipSetDevice(mb->ctx->device));
    return TSQ_OK;
}
}  // namespace

TSQ_API tsq_status tsq_membuf_scan(tsq_membuf* mb, const uint8_t* range_bytes, const int64_t* range_offsets, int64_t n_ranges, uint32_t data_flags, int32_t desc,
                                   tsq_membuf_scan_result* result, int64_t* range_counts) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &mb->hdr;
    TSQ_TRY(mr_enter(mb, result, sizeof *result));
    if (n_ranges < 0) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: negative count");
    if (n_ranges > 0 && !range_offsets) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    if (n_ranges >= (1LL << 30)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "membuf: 2^30 ranges or more");
    const bool dev = data_flags & TSQ_COL_DEVICE;
    int64_t bytes = 0;
    if (!dev && n_ranges > 0) {  // host offsets: the copy is sized by them, so they are checked here as well
        for (int64_t j = 0; j < 2 * n_ranges; j++)
            if (range_offsets[j] < 0 || range_offsets[j] > range_offsets[j + 1]) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: offsets decrease or leave their buffer");
        bytes = range_offsets[2 * n_ranges];
        if (bytes > 0 && !range_bytes) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    }
    MrBoundArgs a;
    memset(&a, 0, sizeof a);
    const void* d_bytes = nullptr;
    const void* d_offs = nullptr;
    TSQ_TRY(mr_dev_array(mb, mb->mr_rng, range_bytes, (size_t)bytes, dev, &d_bytes));
    TSQ_TRY(mr_dev_array(mb, mb->mr_roff, range_offsets, (size_t)(2 * n_ranges + 1) * 8, dev, &d_offs));
    a.bytes = (const uint8_t*)d_bytes, a.offs = (const int64_t*)d_offs, a.n = n_ranges, a.points = 0;
    return mr_scan(mb, a, desc, result, range_counts);
}

TSQ_API tsq_status tsq_membuf_scan_points(tsq_membuf* mb, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n, uint32_t data_flags,
                                          tsq_membuf_scan_result* result) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &mb->hdr;
    TSQ_TRY(mr_enter(mb, result, sizeof *result));
    if (n < 0 || key_bytes < 0) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: negative count");
    if (n > 0 && key_bytes > 0 && !keys) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    if (n > 0 && !key_offsets && key_bytes % n != 0) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: keys of a fixed length need key_bytes to be a multiple of n");
    if (n >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "membuf: 2^31 scan positions or more");
    const bool dev = data_flags & TSQ_COL_DEVICE;
    MrBoundArgs a;
    memset(&a, 0, sizeof a);
    const void* d_bytes = nullptr;
    const void* d_offs = nullptr;
    if (n > 0) {
        TSQ_TRY(mr_dev_array(mb, mb->mr_rng, keys, (size_t)key_bytes, dev, &d_bytes));
        TSQ_TRY(mr_dev_array(mb, mb->mr_roff, key_offsets, ((size_t)n + 1) * 8, dev, &d_offs));
    }
    a.bytes = (const uint8_t*)d_bytes, a.offs = (const int64_t*)d_offs, a.fixed_len = key_offsets || n == 0 ? 0 : key_bytes / n, a.key_bytes = key_bytes;
    a.n = n, a.points = 1;
    return mr_scan(mb, a, 0, result, nullptr);
}

TSQ_API tsq_status tsq_membuf_fetch(tsq_membuf* mb, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* values, int64_t value_cap,
                                    int64_t* value_offsets) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &mb->hdr;
    if (!mb->finished || !mb->mr_have) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: fetch without a preceding scan");
    if (!key_offsets || !value_offsets) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    if (key_cap < mb->mr_key_bytes || value_cap < mb->mr_value_bytes) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: fetch buffer too small");
    if ((mb->mr_key_bytes > 0 && !keys) || (mb->mr_value_bytes > 0 && !values)) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    tsq_ctx* ctx = mb->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    if (mb->mr_pairs == 0) {
        TSQ_HIP(h, hipMemsetAsync(key_offsets, 0, 8, ctx->stream));
        TSQ_HIP(h, hipMemsetAsync(value_offsets, 0, 8, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        return TSQ_OK;
    }
    MrCopyArgs c;
    memset(&c, 0, sizeof c);
    mr_buffer_view(mb, &c.b);
    c.ovals = mb->ovals.as<uint8_t>();
    c.okey_bytes = mb->okey_bytes, c.oval_bytes = mb->oval_bytes;
    c.entry = mb->mr_entry.as<int32_t>(), c.ord = mb->mr_ord.as<int64_t>(), c.koff = mb->mr_koff.as<int64_t>(), c.voff = mb->mr_voff.as<int64_t>();
    c.positions = mb->mr_positions, c.n_pairs = mb->mr_pairs, c.key_bytes = mb->mr_key_bytes, c.value_bytes = mb->mr_value_bytes;
    c.desc = mb->mr_desc;
    c.wave_copy = tsq_knob(ctx, TSQ_KNOB_ROWENC_WAVE_COPY, TSQ_MR_DEFAULT_WAVE_COPY);
    c.keys = keys, c.key_offsets = key_offsets, c.values = values, c.value_offsets = value_offsets;
    hipLaunchKernelGGL(k_mr_copy, dim3(tsq_grid_for(ctx, c.positions, 256)), dim3(256), 0, ctx->stream, c);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_membuf_dirty(tsq_membuf* mb, int64_t table_id, int64_t* n_added, int64_t* n_deleted) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &mb->hdr;
    if (!n_added || !n_deleted) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL result");
    *n_added = *n_deleted = 0;
    if (!mb->finished) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: not finished");
    tsq_ctx* ctx = mb->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    mb->dt_have = false;
    // the table's record range as a range list of one
    uint8_t rng[22];
    const int64_t roffs[3] = {0, 11, 22};
    tsq_mr_record_bound(table_id, 0, rng);
    tsq_mr_record_bound(table_id, 1, rng + 11);
    DevBuf d_rng, d_roff, d_lo, d_cnt, d_ctl, tmp;
    StreamDrain drain(ctx->stream);  // every exit waits for the kernels that use them
    TSQ_TRY(d_rng.reserve(ctx, h, 64));
    TSQ_TRY(d_roff.reserve(ctx, h, 64));
    TSQ_TRY(d_lo.reserve(ctx, h, 64));
    TSQ_TRY(d_cnt.reserve(ctx, h, 64));
    TSQ_TRY(d_ctl.reserve(ctx, h, sizeof(MrCtl) + 64));
    TSQ_HIP(h, hipMemcpyAsync(d_rng.p, rng, sizeof rng, hipMemcpyHostToDevice, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(d_roff.p, roffs, sizeof roffs, hipMemcpyHostToDevice, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(d_ctl.p, 0, sizeof(MrCtl), ctx->stream));
    MrBoundArgs a;
    memset(&a, 0, sizeof a);
    mr_buffer_view(mb, &a.b);
    a.bytes = d_rng.as<uint8_t>(), a.offs = d_roff.as<int64_t>(), a.n = 1, a.points = 0;
    a.rlo = d_lo.as<int64_t>(), a.rcnt = d_cnt.as<int64_t>(), a.ctl = d_ctl.as<MrCtl>();
    hipLaunchKernelGGL(k_mr_bounds, dim3(1), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    int64_t lo = 0, positions = 0;
    TSQ_HIP(h, hipMemcpyAsync(&lo, a.rlo, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&positions, a.rcnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (lo < 0 || positions < 0 || lo + positions > mb->m) return tsq_fail(h, TSQ_ERR_HIP, "internal: the record range of a table leaves the transaction buffer");
    int64_t tot[2] = {0, 0};
    if (positions > 0) {
        TSQ_TRY(mb->dt_handle.reserve(ctx, h, (size_t)positions * 8 + 64));
        TSQ_TRY(mb->dt_added.reserve(ctx, h, ((size_t)positions + 1) * 8 + 64));
        TSQ_TRY(mb->dt_deleted.reserve(ctx, h, ((size_t)positions + 1) * 8 + 64));
        MrDirtyArgs d;
        memset(&d, 0, sizeof d);
        d.b = a.b, d.lo = lo, d.positions = positions;
        d.handle = mb->dt_handle.as<int64_t>(), d.added = mb->dt_added.as<int64_t>(), d.deleted = mb->dt_deleted.as<int64_t>();
        d.ctl = a.ctl;
        hipLaunchKernelGGL(k_mr_dirty_mark, dim3(tsq_grid_for(ctx, positions, 256)), dim3(256), 0, ctx->stream, d);
        TSQ_HIP(h, hipGetLastError());
        TSQ_TRY(tsq_launch_scan64(ctx, h, d.added, positions, tmp));
        TSQ_TRY(tsq_launch_scan64(ctx, h, d.deleted, positions, tmp));
        MrCtl ctl;
        memset(&ctl, 0, sizeof ctl);
        TSQ_HIP(h, hipMemcpyAsync(&tot[0], d.added + positions, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(&tot[1], d.deleted + positions, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(&ctl, d_ctl.p, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        if (ctl.err) return tsq_fail(h, TSQ_ERR_INVALID, "invalid key");
        if (tot[0] < 0 || tot[1] < 0 || tot[0] + tot[1] > positions) return tsq_fail(h, TSQ_ERR_HIP, "internal: the dirty-handle counts are out of range");
    }
    mb->dt_have = true;
    mb->dt_positions = positions;
    *n_added = mb->dt_n_added = tot[0];
    *n_deleted = mb->dt_n_deleted = tot[1];
    return TSQ_OK;
}

TSQ_API tsq_status tsq_membuf_dirty_fetch(tsq_membuf* mb, int64_t* added_out, int64_t* deleted_out) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &mb->hdr;
    if (!mb->finished || !mb->dt_have) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: dirty_fetch without a preceding dirty");
    if ((mb->dt_n_added > 0 && !added_out) || (mb->dt_n_deleted > 0 && !deleted_out)) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    if (mb->dt_n_added + mb->dt_n_deleted == 0) return TSQ_OK;
    tsq_ctx* ctx = mb->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    MrDirtyArgs d;
    memset(&d, 0, sizeof d);
    d.positions = mb->dt_positions;
    d.handle = mb->dt_handle.as<int64_t>(), d.added = mb->dt_added.as<int64_t>(), d.deleted = mb->dt_deleted.as<int64_t>();
    d.n_added = mb->dt_n_added, d.n_deleted = mb->dt_n_deleted;
    d.added_out = added_out, d.deleted_out = deleted_out;
    hipLaunchKernelGGL(k_mr_dirty_write, dim3(tsq_grid_for(ctx, d.positions, 256)), dim3(256), 0, ctx->stream, d);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}
