// tsq_lookup.hip — the storage side of IndexLookUpExecutor's table worker on the GPU (gfx950): a task's handles -> the rows of the
// table that exist (executor/distsql.go:558-637), and the gather of those rows' stored values into the contiguous values / offsets
// form tsq_rowcodec_decode reads (include/tsq.h "IndexLookUp").
//
// tsq_lookup_create (once per table):
//   K18a k_lk_ascending : one streaming pass, handles[i] < handles[i + 1] as signed int64 — what keeps every later index meaningful
//   K18b k_lk_sample    : level k + 1 of the search index = every 2^shift-th entry of level k (tsq_lookup_dp.h)
// tsq_lookup_task (per task):
//        (keep_order = 0) the task's handles are sorted ascending by the radix passes of tsq_sort.hip (a one-column tsq_sort handle:
//        k_sort_image / k_sort_tilehist / k_sort_scan_* / k_sort_scatter); no second sort is written here
//   K18c k_lk_search    : the top level of the index staged in LDS once per workgroup; per handle the lower bound there, the descent
//                         through the sampled levels (L2 / Infinity Cache resident) and the last `shift` steps inside one run of the
//                         table, then the equality test -> row ordinal or -1; per-wave hit counts.  Neighbouring lanes of a sorted
//                         task read the same lines of every level, so one line fetch serves the wave
//        k_compact_scan (tsq_compact.h): the counts -> exclusive bases + the total
//   K18d k_lk_scatter   : ballot + popcount prefix inside every wave's run -> (row, handle) of the hits, in task order
// tsq_rows_gather:
//   K18e k_rg_len       : per listed row the range check of the row index and of its offset pair, and its length
//        tsq_launch_scan64: lengths -> output offsets + the total
//   K18f k_rg_copy      : the bytes; the lane that owns a row copies it (tsq_copy_cell), rows of at least TSQ_KNOB_GATHER_WAVE_COPY
//                         bytes are copied by the whole wave, consecutive lanes on consecutive bytes
#include "tsq_compact.h"
#include "tsq_stage.h"
#include "tsq_lookup_dp.h"

#include <memory>

#define TSQ_LK_DEFAULT_SHIFT 4      // TSQ_KNOB_LOOKUP_STRIDE: the fastest stride of the sweep (profiles/index_lookup_ab.txt)
#define TSQ_RG_DEFAULT_WAVE_COPY 64 // TSQ_KNOB_GATHER_WAVE_COPY

__global__ void __launch_bounds__(256) k_lk_ascending(const int64_t* t, int64_t n, unsigned int* bad) {
    bool b = false;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i + 1 < n; i += (int64_t)gridDim.x * blockDim.x) b = b || !(t[i] < t[i + 1]);
    if (__any(b) && (threadIdx.x & 63) == 0) atomicOr(bad, 1u);
}
__global__ void __launch_bounds__(256) k_lk_sample(const int64_t* src, int64_t n_src, int shift, int64_t* dst, int64_t n_dst) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < n_dst; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t s = tsq_lk_sample_src(j, shift);
        if (s < n_src) dst[j] = src[s];
    }
}

struct LkTaskArgs {
    tsq_lk_index ix;
    const int64_t* handles;          // the task's handles (sorted for keep_order = 0)
    int64_t n;
    int64_t rows_per_wave;           // a multiple of 64
    int64_t* pos;                    // [n]: row ordinal or -1
    unsigned long long* block_base;  // per-wave counts -> exclusive bases
    unsigned long long* total;
    int64_t* rows_out;               // [n]
    int64_t* handles_out;            // [n]
    int32_t top_in_lds;
};
__global__ void __launch_bounds__(256) k_lk_search(LkTaskArgs a) {
    __shared__ int64_t s_top[TSQ_LK_TOP_MAX];
    const int64_t* top = a.ix.lv[a.ix.levels];
    if (a.top_in_lds) {  // (workgroup uniform; n[levels] <= TSQ_LK_TOP_MAX is the host's condition for it)
        const int64_t nt = a.ix.n[a.ix.levels] < TSQ_LK_TOP_MAX ? a.ix.n[a.ix.levels] : TSQ_LK_TOP_MAX;
        for (int64_t i = threadIdx.x; i < nt; i += 256) s_top[i] = top[i];
        __syncthreads();
        top = s_top;
    }
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = u * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.n ? hi : a.n;
    unsigned int c = 0;
    for (int64_t r = lo + lane; r < hi; r += 64) {
        const int64_t p = tsq_lk_find(a.ix, top, a.handles[r]);
        a.pos[r] = p;
        c += p >= 0 ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) a.block_base[u] = c;
}
__global__ void __launch_bounds__(256) k_lk_scatter(LkTaskArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = u * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.n ? hi : a.n;
    unsigned long long cur = a.block_base[u];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t r0 = lo; r0 < hi; r0 += 64) {  // (wave uniform trip count: lo and hi are)
        const int64_t r = r0 + lane;
        const int64_t p = r < hi ? a.pos[r] : -1;
        const bool hit = p >= 0;
        const unsigned long long bal = __ballot(hit);
        const unsigned long long at = cur + (unsigned long long)__popcll(bal & lt);
        if (hit && at < (unsigned long long)a.n) {
            a.rows_out[at] = p;
            a.handles_out[at] = a.handles[r];
        }
        cur += (unsigned long long)__popcll(bal);
    }
}

__global__ void __launch_bounds__(256) k_rg_len(RgArgs a) {
    unsigned int e = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = a.rows[i];
        int64_t len = 0;
        if (r < 0 || r >= a.n_src_rows) {
            e |= 1u;
        } else {
            const int64_t b = a.offsets[r], t = a.offsets[r + 1];
            if (b < 0 || t < b || t > a.n_bytes) e |= 2u;
            else len = t - b;
        }
        a.lens[i] = len;
    }
    if (e) atomicOr(a.err, e);
}
// one row per lane and step; the rows of a step that reach the threshold are then copied one after the other by the 64 lanes
__global__ void __launch_bounds__(256) k_rg_copy(RgArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r0 = wave * 64; r0 < a.n; r0 += nwaves * 64) {  // (wave uniform)
        const int64_t i = r0 + lane;
        const bool in = i < a.n;
        const int64_t o0 = in ? a.lens[i] : 0, o1 = in ? a.lens[i + 1] : 0;
        const int64_t len = o1 - o0;
        if (in) {
            a.out_offsets[i + 1] = o1;
            if (i == 0) a.out_offsets[0] = 0;
        }
        const uint8_t* s = a.values;
        if (in && len > 0) s = a.values + a.offsets[a.rows[i]];  // (k_rg_len checked both; len > 0 only for a checked row)
        uint8_t* d = a.out + o0;
        const bool by_wave = a.wave_copy > 0 && len >= a.wave_copy;
        if (in && len > 0 && !by_wave) tsq_copy_cell(d, s, len);
        unsigned long long todo = __ballot(in && len > 0 && by_wave);
        while (todo) {  // (wave uniform)
            const int src_lane = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const uint8_t* ws = (const uint8_t*)__shfl((unsigned long long)s, src_lane, 64);
            uint8_t* wd = (uint8_t*)__shfl((unsigned long long)d, src_lane, 64);
            const int64_t wn = (int64_t)__shfl((unsigned long long)len, src_lane, 64);
            for (int64_t b = lane; b < wn; b += 64) wd[b] = ws[b];
        }
    }
}

// (declared in tsq_lookup_dp.h) the copy pass alone, for tsq_mvcc.hip: its pairs leave through the same kernel, lengths already scanned
tsq_status tsq_launch_rg_copy(tsq_ctx* ctx, tsq_handle_hdr* h, const RgArgs& a) {
    hipLaunchKernelGGL(k_rg_copy, dim3(tsq_grid_for(ctx, a.n, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    return TSQ_OK;
}

// ====================================================================== host side
#define TSQ_MAGIC_LOOKUP 0x7473714cu /* 'tsqL' */

struct tsq_lookup {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    std::atomic<int> cancelled{0};
    tsq_lk_index ix;
    DevBuf level[TSQ_LK_MAX_LEVELS + 1];  // level[0]: the library's copy of the table's handles
    DevBuf in_handles, sorted, sorted_bm, pos, base, out_rows, out_handles;
    int64_t tasks = 0, handles = 0, found = 0;
    double kernel_ms = 0;
    DevEvent ev[2];
};

namespace {
tsq_status lk_cancelled(tsq_lookup* l) {
    if (l->cancelled.load()) return tsq_fail(&l->hdr, TSQ_ERR_CANCELLED, "lookup cancelled");
    return TSQ_OK;
}
// the task's handles (device, n of them) sorted ascending as signed int64 into l->sorted, by the radix passes of tsq_sort.hip
tsq_status lk_sort(tsq_lookup* l, const int64_t* dev_handles, int64_t n) {
    tsq_ctx* ctx = l->ctx;
    tsq_handle_hdr* h = &l->hdr;
    TSQ_TRY(l->sorted.reserve(ctx, h, (size_t)n * 8 + 64));
    TSQ_TRY(l->sorted_bm.reserve(ctx, h, tsq_bitmap_bytes(n) + 64));
    tsq_sort_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_cols = 1;
    cfg.col_types[0] = TSQ_I64;
    cfg.n_keys = 1;
    cfg.limit_count = -1;
    cfg.max_chunk_size = 1024;
    tsq_sort* s = nullptr;
    tsq_status st = tsq_sort_create(ctx, &cfg, &s);
    if (st != TSQ_OK) return tsq_fail(h, st, std::string("lookup: sort: ") + tsq_last_error(ctx));
    tsq_col in, out;
    memset(&in, 0, sizeof in);
    in.data = (void*)dev_handles;
    in.length = n;
    in.elem_size = 8;
    in.type = TSQ_I64;
    in.flags = TSQ_COL_DEVICE;
    out = in;
    out.data = l->sorted.p;
    out.null_bitmap = l->sorted_bm.as<uint8_t>();
    int64_t got = 0;
    int32_t eos = 0;
    st = tsq_sort_push(s, &in, 1, n);
    if (st == TSQ_OK) st = tsq_sort_finish(s);
    if (st == TSQ_OK) st = tsq_sort_pull(s, &out, 1, n, &got, &eos);
    if (st != TSQ_OK) tsq_fail(h, st, std::string("lookup: sort: ") + tsq_last_error(s));
    else if (got != n) st = tsq_fail(h, TSQ_ERR_HIP, "internal: the sort of the task's handles lost rows");
    tsq_sort_destroy(s);
    return st;
}
}  // namespace

// (declared in tsq_lookup_dp.h) for tsq_dupcheck.hip: a kernel there runs the same descent per row (tsq_lk_find) without a second copy
const tsq_lk_index* tsq_lookup_index_of(const tsq_lookup* l) { return &l->ix; }

TSQ_API tsq_status tsq_lookup_create(tsq_ctx* ctx, const int64_t* table_handles, int64_t n_rows, uint32_t data_flags, tsq_lookup** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !out) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_lookup_create: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (n_rows < 0 || (n_rows > 0 && !table_handles)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_lookup_create: bad handle array");
    if (!(data_flags & TSQ_COL_DEVICE)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_lookup_create: the table's handles must be device resident (TSQ_COL_DEVICE)");
    std::unique_ptr<tsq_lookup> l(new tsq_lookup());
    l->hdr.magic = TSQ_MAGIC_LOOKUP;
    l->ctx = ctx;
    memset(&l->ix, 0, sizeof l->ix);
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    const int shift = (int)tsq_knob(ctx, TSQ_KNOB_LOOKUP_STRIDE, TSQ_LK_DEFAULT_SHIFT);
    tsq_lk_plan(&l->ix, n_rows, shift, TSQ_LK_TOP_MAX);
    tsq_status st = TSQ_OK;
    hipError_t e = hipSuccess;
    for (int i = 0; i < 2 && st == TSQ_OK; i++)
        if (l->ev[i].create() != hipSuccess) st = tsq_fail(ch, TSQ_ERR_HIP, "hipEventCreate");
    if (st == TSQ_OK) st = l->level[0].reserve(ctx, ch, (size_t)n_rows * 8 + 64);
    l->ix.lv[0] = l->level[0].as<int64_t>();
    if (st == TSQ_OK && n_rows > 0) {
        unsigned int* bad = (unsigned int*)(ctx->dscratch + 16);
        e = hipMemcpyAsync(l->level[0].p, table_handles, (size_t)n_rows * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 8, ctx->stream);
        if (e == hipSuccess) {
            hipLaunchKernelGGL(k_lk_ascending, dim3(tsq_grid_for(ctx, n_rows, 256, 4)), dim3(256), 0, ctx->stream, l->ix.lv[0], n_rows, bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned + 40, bad, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && (ctx->pinned[40] & 1u)) st = tsq_fail(ch, TSQ_ERR_INVALID, "table handles not ascending");
        for (int k = 1; k <= l->ix.levels && st == TSQ_OK && e == hipSuccess; k++) {
            st = l->level[k].reserve(ctx, ch, (size_t)l->ix.n[k] * 8 + 64);
            if (st != TSQ_OK) break;
            l->ix.lv[k] = l->level[k].as<int64_t>();
            hipLaunchKernelGGL(k_lk_sample, dim3(tsq_grid_for(ctx, l->ix.n[k], 256)), dim3(256), 0, ctx->stream, l->ix.lv[k - 1], l->ix.n[k - 1],
                               l->ix.shift, l->level[k].as<int64_t>(), l->ix.n[k]);
            e = hipGetLastError();
        }
        if (st == TSQ_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (st == TSQ_OK && e != hipSuccess) st = tsq_fail(ch, TSQ_ERR_HIP, std::string("tsq_lookup_create: ") + hipGetErrorString(e));
    }
    if (st != TSQ_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return st;
    }
    *out = l.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_lookup_task(tsq_lookup* l, const int64_t* handles, int64_t n, uint32_t data_flags, int32_t keep_order, int64_t* rows_out,
                                   int64_t* handles_out, int64_t* n_found) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(l, TSQ_MAGIC_LOOKUP));
    if (!l || l->hdr.magic != TSQ_MAGIC_LOOKUP) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &l->hdr;
    if (n_found) *n_found = 0;
    TSQ_TRY(lk_cancelled(l));
    if (!n_found || n < 0 || (n > 0 && (!handles || !rows_out || !handles_out))) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_lookup_task: bad arguments");
    if (n >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "lookup: 2^31 handles or more in one task");
    l->tasks++;
    l->handles += n;
    if (n == 0 || l->ix.n[0] == 0) return TSQ_OK;
    tsq_ctx* ctx = l->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool dev = data_flags & TSQ_COL_DEVICE;
    const int64_t* src = handles;
    if (!dev) {
        TSQ_TRY(l->in_handles.reserve(ctx, h, (size_t)n * 8 + 64));
        TSQ_HIP(h, hipMemcpyAsync(l->in_handles.p, handles, (size_t)n * 8, hipMemcpyHostToDevice, ctx->stream));
        src = l->in_handles.as<int64_t>();
    }
    TSQ_HIP(h, hipEventRecord(l->ev[0], ctx->stream));
    if (!keep_order) {
        TSQ_TRY(lk_sort(l, src, n));
        src = l->sorted.as<int64_t>();
    }
    LkTaskArgs a;
    memset(&a, 0, sizeof a);
    a.ix = l->ix;
    a.handles = src;
    a.n = n;
    a.top_in_lds = l->ix.n[l->ix.levels] <= TSQ_LK_TOP_MAX ? 1 : 0;
    const int grid = tsq_grid_for(ctx, n, 256);
    const int n_runs = grid * 4;
    a.rows_per_wave = (((n + n_runs - 1) / n_runs) + 63) & ~(int64_t)63;
    TSQ_TRY(l->pos.reserve(ctx, h, (size_t)n * 8 + 64));
    TSQ_TRY(l->base.reserve(ctx, h, (size_t)n_runs * 8 + 64));
    a.pos = l->pos.as<int64_t>();
    a.block_base = l->base.as<unsigned long long>();
    a.total = a.block_base + n_runs;
    if (dev) {
        a.rows_out = rows_out;
        a.handles_out = handles_out;
    } else {
        TSQ_TRY(l->out_rows.reserve(ctx, h, (size_t)n * 8 + 64));
        TSQ_TRY(l->out_handles.reserve(ctx, h, (size_t)n * 8 + 64));
        a.rows_out = l->out_rows.as<int64_t>();
        a.handles_out = l->out_handles.as<int64_t>();
    }
    hipLaunchKernelGGL(k_lk_search, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, a.block_base, n_runs, a.total);
    hipLaunchKernelGGL(k_lk_scatter, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 41, a.total, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipEventRecord(l->ev[1], ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t nf = std::min<int64_t>(n, (int64_t)ctx->pinned[41]);
    if (!dev && nf > 0) {
        TSQ_HIP(h, hipMemcpyAsync(rows_out, a.rows_out, (size_t)nf * 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(handles_out, a.handles_out, (size_t)nf * 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    }
    float ms = 0;
    if (hipEventElapsedTime(&ms, l->ev[0], l->ev[1]) == hipSuccess) l->kernel_ms += ms;
    l->found += nf;
    *n_found = nf;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_lookup_stats(tsq_lookup* l, int64_t* tasks, int64_t* handles, int64_t* found, double* kernel_ms) {
    if (!l || l->hdr.magic != TSQ_MAGIC_LOOKUP) return TSQ_ERR_INVALID;
    if (tasks) *tasks = l->tasks;
    if (handles) *handles = l->handles;
    if (found) *found = l->found;
    if (kernel_ms) *kernel_ms = l->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_lookup_cancel(tsq_lookup* l) {
    if (!l || l->hdr.magic != TSQ_MAGIC_LOOKUP) return TSQ_ERR_INVALID;
    l->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_lookup_destroy(tsq_lookup* l) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(l, TSQ_MAGIC_LOOKUP));
    if (!l || l->hdr.magic != TSQ_MAGIC_LOOKUP) return;
    (void)hipSetDevice(l->ctx->device);
    (void)hipStreamSynchronize(l->ctx->stream);
    l->hdr.magic = 0;
    delete l;
}

TSQ_API tsq_status tsq_rows_gather(tsq_ctx* ctx, const uint8_t* values, int64_t n_bytes, const int64_t* offsets, int64_t n_src_rows, const int64_t* rows,
                                   int64_t n, uint8_t* out, int64_t cap_bytes, int64_t* out_offsets, int64_t* bytes_out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (bytes_out) *bytes_out = 0;
    if (!bytes_out || n < 0 || n_src_rows < 0 || n_bytes < 0 || cap_bytes < 0 || (cap_bytes > 0 && (!out || !out_offsets)) || (n > 0 && (!rows || !offsets)) ||
        (n_bytes > 0 && !values))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_gather: bad arguments");
    if (n >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_rows_gather: 2^31 rows or more");
    TSQ_HIP(h, hipSetDevice(ctx->device));
    if (n == 0) {
        if (out_offsets) {
            TSQ_HIP(h, hipMemsetAsync(out_offsets, 0, 8, ctx->stream));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        }
        return TSQ_OK;
    }
    DevBuf lens, scratch;
    StreamDrain drain(ctx->stream);  // every exit below waits for the kernels that read the two buffers
    TSQ_TRY(lens.reserve(ctx, h, ((size_t)n + 1) * 8 + 64));
    RgArgs a;
    memset(&a, 0, sizeof a);
    a.values = values;
    a.n_bytes = n_bytes;
    a.offsets = offsets;
    a.n_src_rows = n_src_rows;
    a.rows = rows;
    a.n = n;
    a.lens = lens.as<int64_t>();
    a.err = (unsigned int*)(ctx->dscratch + 16);
    a.wave_copy = tsq_knob(ctx, TSQ_KNOB_GATHER_WAVE_COPY, TSQ_RG_DEFAULT_WAVE_COPY);
    hipError_t e = hipMemsetAsync(a.err, 0, 8, ctx->stream);
    if (e == hipSuccess) {
        hipLaunchKernelGGL(k_rg_len, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
        e = hipGetLastError();
    }
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_rows_gather: ") + hipGetErrorString(e));
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.lens, n, scratch));
    e = hipMemcpyAsync(ctx->pinned + 40, a.err, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned + 41, a.lens + n, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_rows_gather: ") + hipGetErrorString(e));
    const unsigned int err = (unsigned int)ctx->pinned[40];
    if (err & 1u) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_gather: row index out of range");
    if (err & 2u) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_gather: row index out of range of the values (offsets must not decrease)");
    const int64_t total = (int64_t)ctx->pinned[41];
    *bytes_out = total;
    if (total > cap_bytes) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_gather: output buffer too small (*bytes_out = bytes needed)");
    if (!out_offsets) return TSQ_OK;  // a size query that found nothing to write
    a.out = out;
    a.out_offsets = out_offsets;
    hipLaunchKernelGGL(k_rg_copy, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, std::string("tsq_rows_gather: ") + hipGetErrorString(e));
    return TSQ_OK;
}
