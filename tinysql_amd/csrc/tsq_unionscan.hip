// tsq_unionscan.hip — UnionScanExec on the GPU (gfx950): the dirty-handle filter and the ordered two-way merge of the kept snapshot
// rows with the transaction's added rows (executor/union_scan.go:89-300; include/tsq.h "UnionScan").
//
// One push = one self-contained step (the streaming rule of the header):
//   K17a k_us_probe   : per snapshot row, probe the handle set -> a keep flag; per-wave keep counts     (skipped: empty set)
//        k_compact_scan (tsq_compact.h): the counts -> exclusive bases + the total
//   K17b k_us_scatter : ballot + popcount prefix inside every wave's run -> the kept-row list, in input order
//   K17c k_us_bound   : one lane: how many added rows (from the cursor) precede the last kept row -> m of this push
//   K17d k_us_merge   : merge path over the output diagonal of (kept rows, next m added rows), two steps in one launch: the first two
//                       lanes of a workgroup search the splits of its tile's two boundaries over the whole runs; then every lane
//                       searches its own diagonal inside the tile's two stretches (at most TSQ_US_TILE rows each: a few cache lines
//                       the workgroup shares) and emits TSQ_US_LANE outputs sequentially into the take list (side bit + row)
//   K17e k_us_gather  : fixed-width cells and NOT-NULL flags of every column by the take list, into the output queue
//   K17f k_us_var_len / k_us_var_copy : var-len columns — lengths, scan (tsq_launch_scan64), bytes — as k_sort_var_len / _copy
// A pull copies the head of the queue out (the NOT-NULL flags are packed into the bitmap there).
//
// ONE merge route is written, the general one: the comparator (tsq_unionscan_dp.h) reads the key cells and the handle from global
// memory, for any number and type of index columns; nothing is staged in LDS but the two splits of a tile.  The LDS route for
// (NULL digit, one image, handle) tuples is not written (DESIGN.md §5 says what that costs).
#include "tsq_compact.h"
#include "tsq_stage.h"
#include "tsq_unionscan_dp.h"

#include <memory>

#define TSQ_US_LANE 8                    // outputs per lane of k_us_merge
#define TSQ_US_TILE (256 * TSQ_US_LANE)  // outputs per tile (one workgroup): 2048

struct UsFilterArgs {
    const int64_t* handles;  // the handle column of the pushed chunk (raw 8 bytes)
    int64_t nrows;
    tsq_us_set set;
    uint8_t* keep;                   // one byte per row
    int64_t rows_per_wave;           // a multiple of 64
    unsigned long long* block_base;  // per-wave counts -> exclusive bases
    unsigned long long* total;
    uint32_t* kept_rows;             // [nrows]
};
__global__ void __launch_bounds__(256) k_us_probe(UsFilterArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = u * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.nrows ? hi : a.nrows;
    unsigned int c = 0;
    for (int64_t r = lo + lane; r < hi; r += 64) {
        const bool keep = !tsq_us_set_has(a.set, (uint64_t)a.handles[r]);
        a.keep[r] = keep ? 1 : 0;
        c += keep ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) a.block_base[u] = c;
}
__global__ void __launch_bounds__(256) k_us_scatter(UsFilterArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = u * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.nrows ? hi : a.nrows;
    unsigned long long cur = a.block_base[u];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t r0 = lo; r0 < hi; r0 += 64) {  // (wave uniform trip count: lo and hi are)
        const int64_t r = r0 + lane;
        const bool keep = r < hi && a.keep[r];
        const unsigned long long bal = __ballot(keep);
        const unsigned long long at = cur + (unsigned long long)__popcll(bal & lt);
        if (keep && at < (unsigned long long)a.nrows) a.kept_rows[at] = (uint32_t)r;
        cur += (unsigned long long)__popcll(bal);
    }
}

// tsq_unionscan_create_dev: the handle set built on the device, without a compare.  Every handle, duplicates included, claims the first
// unoccupied slot on its probe path with an atomicOr on the occupancy word; only the claimer writes the key; the kernel boundary orders
// the build before any probe.  At least twice as many slots as handles: a free slot is always met.  (occ zeroed by the host.)
struct UsBuildArgs {
    const int64_t* added;
    int64_t n_added;
    const int64_t* deleted;
    int64_t n_deleted;
    uint64_t* keys;
    uint32_t* occ;
    uint64_t slots;
};
__global__ void __launch_bounds__(256) k_us_build(UsBuildArgs a) {
    const int64_t n = a.n_added + a.n_deleted;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint64_t handle = (uint64_t)(i < a.n_added ? a.added[i] : a.deleted[i - a.n_added]);
        uint64_t s = tsq_us_slot(handle, a.slots);
        for (uint64_t step = 0; step < a.slots; step++) {  // (bounded by the table size, as the probe's walk)
            const uint32_t bit = 1u << (s & 31);
            if (!(atomicOr(&a.occ[s >> 5], bit) & bit)) {
                a.keys[s] = handle;
                break;
            }
            s = (s + 1) & (a.slots - 1);
        }
    }
}

struct UsMergeArgs {
    tsq_us_order order;
    tsq_us_run S, A;                  // S.v.n / A.v.n are set by the host for k_us_merge; k_us_bound reads the kept count from n_kept
    const unsigned long long* n_kept; // k_us_bound: the filter's total (null: S.v.n)
    unsigned long long* m_out;        // k_us_bound
    uint32_t* take;                   // [S.v.n + A.v.n]
};
__global__ void k_us_bound(UsMergeArgs a) {
    if (blockIdx.x != 0 || threadIdx.x != 0) return;
    int64_t nk = a.n_kept ? (int64_t)*a.n_kept : a.S.v.n;
    nk = nk < 0 ? 0 : (nk > a.S.v.n ? a.S.v.n : nk);  // S.v.n = the rows of the push here: the list cannot be longer
    *a.m_out = nk == 0 ? 0ull : (unsigned long long)tsq_us_bound(a.order, a.A.cs, a.A.v, a.S.cs, tsq_us_phys(a.S.v, nk - 1));
}
__global__ void __launch_bounds__(256) k_us_merge(UsMergeArgs a) {
    __shared__ int64_t s_split[2];
    const int64_t total = a.S.v.n + a.A.v.n;
    const int64_t ntiles = (total + TSQ_US_TILE - 1) / TSQ_US_TILE;
    for (int64_t tile = blockIdx.x; tile < ntiles; tile += gridDim.x) {
        const int64_t d0 = tile * TSQ_US_TILE, d1 = d0 + TSQ_US_TILE < total ? d0 + TSQ_US_TILE : total;
        if (threadIdx.x < 2) s_split[threadIdx.x] = tsq_us_diag(a.order, a.S.cs, a.S.v, a.A.cs, a.A.v, threadIdx.x ? d1 : d0);
        __syncthreads();
        tsq_us_view s, v;
        tsq_us_tile_views(a.S.v, a.A.v, d0, d1, s_split[0], s_split[1], &s, &v);
        const int64_t d = (int64_t)threadIdx.x * TSQ_US_LANE;
        if (d < s.n + v.n) {  // (take + d0: the tile's outputs; s.n + v.n <= d1 - d0)
            const int64_t i = tsq_us_diag(a.order, a.S.cs, s, a.A.cs, v, d);
            tsq_us_lane_merge(a.order, a.S.cs, s, a.A.cs, v, d, i, TSQ_US_LANE, a.take + d0);
        }
        __syncthreads();
    }
}
// the take list of a run alone (no rows on the other side)
__global__ void __launch_bounds__(256) k_us_take_run(tsq_us_view r, uint32_t side, uint32_t* take) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < r.n; i += (int64_t)gridDim.x * blockDim.x)
        take[i] = side | (uint32_t)tsq_us_phys(r, i);
}

struct UsGatherArgs {
    const uint32_t* take;
    int64_t rows;
    int64_t phys[2];  // physical rows of the two sides: an entry beyond them gives a NULL cell (unsorted input only)
    const void* src[2][TSQ_MAX_COLS];
    const uint8_t* src_nulls[2][TSQ_MAX_COLS];
    void* dst[TSQ_MAX_COLS];        // already offset to the queue's tail
    uint8_t* dst_nn[TSQ_MAX_COLS];  // one byte per row, 1 = NOT NULL
    int32_t es[TSQ_MAX_COLS];       // 8, 4, or 0 for a var-len column (its flags only)
};
// blockIdx.y = column; one output row per lane and step: consecutive lanes write consecutive cells
__global__ void __launch_bounds__(256) k_us_gather(UsGatherArgs a) {
    const int c = blockIdx.y;
    const void* s0 = a.src[0][c];
    const void* s1 = a.src[1][c];
    const uint8_t* n0 = a.src_nulls[0][c];
    const uint8_t* n1 = a.src_nulls[1][c];
    const int es = a.es[c];
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.rows; r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t e = a.take[r];
        const uint32_t side = e >> 31, id = e & 0x7fffffffu;
        const bool in = (int64_t)id < a.phys[side];
        const uint8_t* nulls = side ? n1 : n0;
        const void* src = side ? s1 : s0;
        const bool nn = in && (!nulls || ((nulls[id >> 3] >> (id & 7)) & 1));
        if (es == 8) ((uint64_t*)a.dst[c])[r] = nn ? ((const uint64_t*)src)[id] : 0ull;
        else if (es == 4) ((uint32_t*)a.dst[c])[r] = nn ? ((const uint32_t*)src)[id] : 0u;
        a.dst_nn[c][r] = nn ? 1 : 0;
    }
}

struct UsVarArgs {
    const uint32_t* take;
    int64_t rows;
    int64_t phys[2];
    const int64_t* src_offs[2];
    const uint8_t* src_data[2];
    const uint8_t* src_nulls[2];
    int64_t* lens;       // [rows + 1]: lengths, then (scan) offsets relative to this step's first byte
    int64_t* q_offs;     // the queue's offsets, already at its tail: q_offs[r + 1] = q_bytes + lens[r + 1]
    uint8_t* q_data;     // the queue's data, already at its tail
    int64_t q_bytes;
};
__global__ void __launch_bounds__(256) k_us_var_len(UsVarArgs a) {
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.rows; r += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t e = a.take[r];
        const uint32_t side = e >> 31, id = e & 0x7fffffffu;
        const uint8_t* nulls = a.src_nulls[side];
        const bool ok = (int64_t)id < a.phys[side] && (!nulls || ((nulls[id >> 3] >> (id & 7)) & 1));
        const int64_t n = ok ? a.src_offs[side][id + 1] - a.src_offs[side][id] : 0;  // a NULL cell has no bytes
        a.lens[r] = n > 0 ? n : 0;
    }
}
template <bool WAVE>
__global__ void __launch_bounds__(256) k_us_var_copy(UsVarArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t gtid = (int64_t)blockIdx.x * blockDim.x + threadIdx.x, nthr = (int64_t)gridDim.x * blockDim.x;
    const int64_t first = WAVE ? gtid >> 6 : gtid, step = WAVE ? nthr >> 6 : nthr;
    for (int64_t r = first; r < a.rows; r += step) {
        const int64_t n = a.lens[r + 1] - a.lens[r];
        if (!WAVE || lane == 0) a.q_offs[r + 1] = a.q_bytes + a.lens[r + 1];
        if (n <= 0) continue;
        const uint32_t e = a.take[r];
        const uint32_t side = e >> 31, id = e & 0x7fffffffu;
        const uint8_t* s = a.src_data[side] + a.src_offs[side][id];
        uint8_t* d = a.q_data + a.lens[r];
        if (!WAVE) {
            tsq_copy_cell(d, s, n);
        } else {
            for (int64_t b = lane; b < n; b += 64) d[b] = s[b];
        }
    }
}

// ====================================================================== host side
#define TSQ_MAGIC_UNIONSCAN 0x74737155u /* 'tsqU' */

struct tsq_unionscan {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    tsq_unionscan_cfg cfg;
    std::atomic<int> cancelled{0};
    tsq_us_order order;
    DevBuf set_keys, set_occ;
    uint64_t set_slots = 0;
    std::vector<ColStore> added;  // the added rows
    std::vector<ColStore> snap;   // the chunk of a host push (cleared by the next)
    int64_t n_added = 0, a_cursor = 0;
    bool added_set = false, pushed = false, finished = false;
    // the output queue: rows [cursor, q_rows) wait for a pull; it restarts at 0 once everything has been pulled
    std::vector<DevBuf> q_data, q_nn, q_offs;
    std::vector<int64_t> q_bytes;
    int64_t q_rows = 0, cursor = 0;
    DevBuf keep, kept_rows, base, take, lens, scratch, tmp_bits, tmp_offs;
    std::vector<DevBuf> obm, ooffs;  // pulls into host memory: the packed bitmap / rebased offsets of a column
    std::vector<int64_t> vlo, vbytes;  // var-len columns: first byte and byte count of the rows the last peek sized
    int64_t peek_cursor = -1, peek_rows = 0;
    int64_t snapshot_rows = 0, dropped_rows = 0, added_out = 0;
    double kernel_ms = 0;
    DevEvent ev[2];
};

namespace {
tsq_status us_cancelled(tsq_unionscan* u) {
    if (u->cancelled.load()) return tsq_fail(&u->hdr, TSQ_ERR_CANCELLED, "union scan cancelled");
    return TSQ_OK;
}
void us_fill_run(tsq_us_run& r, const std::vector<ColStore>& cols) { tsq_fill_colset(r.cs, cols); }

// rows of the take list -> the tail of the queue
tsq_status us_emit(tsq_unionscan* u, const tsq_colset& s_cs, int64_t s_phys, int64_t rows) {
    tsq_ctx* ctx = u->ctx;
    tsq_handle_hdr* h = &u->hdr;
    const int n_cols = u->cfg.n_cols;
    tsq_colset a_cs;
    tsq_fill_colset(a_cs, u->added);
    UsGatherArgs g;
    memset(&g, 0, sizeof g);
    g.take = u->take.as<uint32_t>();
    g.rows = rows;
    g.phys[0] = s_phys;
    g.phys[1] = u->n_added;
    const int64_t q0 = u->q_rows;
    for (int c = 0; c < n_cols; c++) {
        const bool var = u->cfg.col_types[c] == TSQ_BYTES;
        const int es = var ? 0 : tsq_elem_size(u->cfg.col_types[c]);
        g.es[c] = es;
        g.src[0][c] = s_cs.data[c];
        g.src[1][c] = a_cs.data[c];
        g.src_nulls[0][c] = s_cs.nulls[c];
        g.src_nulls[1][c] = a_cs.nulls[c];
        if (!var) {
            TSQ_TRY(u->q_data[c].reserve(ctx, h, (size_t)(q0 + rows) * es + 64, true, (size_t)q0 * es));
            g.dst[c] = (char*)u->q_data[c].p + (size_t)q0 * es;
        }
        TSQ_TRY(u->q_nn[c].reserve(ctx, h, (size_t)(q0 + rows) + 64, true, (size_t)q0));
        g.dst_nn[c] = u->q_nn[c].as<uint8_t>() + q0;
    }
    const int gx = tsq_grid_for(ctx, rows, 256);
    hipLaunchKernelGGL(k_us_gather, dim3(gx, n_cols), dim3(256), 0, ctx->stream, g);
    TSQ_HIP(h, hipGetLastError());
    for (int c = 0; c < n_cols; c++) {
        if (u->cfg.col_types[c] != TSQ_BYTES) continue;
        UsVarArgs va;
        memset(&va, 0, sizeof va);
        va.take = g.take;
        va.rows = rows;
        va.phys[0] = g.phys[0];
        va.phys[1] = g.phys[1];
        va.src_offs[0] = s_cs.offs[c];
        va.src_offs[1] = a_cs.offs[c];
        va.src_data[0] = (const uint8_t*)s_cs.data[c];
        va.src_data[1] = (const uint8_t*)a_cs.data[c];
        va.src_nulls[0] = s_cs.nulls[c];
        va.src_nulls[1] = a_cs.nulls[c];
        TSQ_TRY(u->lens.reserve(ctx, h, ((size_t)rows + 1) * 8 + 64));
        va.lens = u->lens.as<int64_t>();
        hipLaunchKernelGGL(k_us_var_len, dim3(gx), dim3(256), 0, ctx->stream, va);
        TSQ_HIP(h, hipGetLastError());
        TSQ_TRY(tsq_launch_scan64(ctx, h, va.lens, rows, u->scratch));
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 48, va.lens + rows, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        const int64_t nbytes = (int64_t)ctx->pinned[48];
        if (nbytes < 0) return tsq_fail(h, TSQ_ERR_INVALID, "var-len column: offsets must not decrease");
        const bool fresh = u->q_offs[c].p == nullptr;
        TSQ_TRY(u->q_offs[c].reserve(ctx, h, (size_t)(q0 + rows + 1) * 8 + 64, true, (size_t)(q0 + 1) * 8));
        if (fresh || q0 == 0) TSQ_HIP(h, hipMemsetAsync(u->q_offs[c].p, 0, 8, ctx->stream));
        TSQ_TRY(u->q_data[c].reserve(ctx, h, (size_t)(u->q_bytes[c] + nbytes) + 64, true, (size_t)u->q_bytes[c]));
        va.q_offs = u->q_offs[c].as<int64_t>() + q0;
        va.q_data = u->q_data[c].as<uint8_t>() + u->q_bytes[c];
        va.q_bytes = u->q_bytes[c];
        if (nbytes / rows > 32) hipLaunchKernelGGL(k_us_var_copy<true>, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, va);
        else hipLaunchKernelGGL(k_us_var_copy<false>, dim3(gx), dim3(256), 0, ctx->stream, va);
        TSQ_HIP(h, hipGetLastError());
        u->q_bytes[c] += nbytes;
    }
    u->q_rows += rows;
    return TSQ_OK;
}

// merge the run S (n_kept logical rows) with the next m added rows into the take list and emit
tsq_status us_merge_emit(tsq_unionscan* u, tsq_us_run& S, int64_t s_phys, int64_t n_kept, int64_t m) {
    tsq_ctx* ctx = u->ctx;
    tsq_handle_hdr* h = &u->hdr;
    const int64_t total = n_kept + m;
    if (total <= 0) return TSQ_OK;
    if (u->cursor == u->q_rows) {  // everything was pulled: the queue restarts
        u->cursor = u->q_rows = 0;
        for (auto& b : u->q_bytes) b = 0;
        u->peek_cursor = -1;
    }
    TSQ_TRY(u->take.reserve(ctx, h, (size_t)total * 4 + 64));
    UsMergeArgs a;
    memset(&a, 0, sizeof a);
    a.order = u->order;
    a.S = S;
    a.S.v.n = n_kept;
    us_fill_run(a.A, u->added);
    a.A.v.base = u->a_cursor;
    a.A.v.n = m;
    a.take = u->take.as<uint32_t>();
    if (m == 0) {
        hipLaunchKernelGGL(k_us_take_run, dim3(tsq_grid_for(ctx, n_kept, 256)), dim3(256), 0, ctx->stream, a.S.v, 0u, a.take);
    } else if (n_kept == 0) {
        hipLaunchKernelGGL(k_us_take_run, dim3(tsq_grid_for(ctx, m, 256)), dim3(256), 0, ctx->stream, a.A.v, TSQ_US_SIDE_ADDED, a.take);
    } else {
        TSQ_HIP(h, hipMemsetAsync(a.take, 0, (size_t)total * 4, ctx->stream));  // (unsorted input may leave entries unwritten)
        hipLaunchKernelGGL(k_us_merge, dim3(tsq_grid_for(ctx, total, 256, TSQ_US_LANE)), dim3(256), 0, ctx->stream, a);  // one tile per workgroup and step
    }
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(us_emit(u, S.cs, s_phys, total));
    u->a_cursor += m;
    u->added_out += m;
    return TSQ_OK;
}

tsq_status us_timed_end(tsq_unionscan* u) {
    tsq_ctx* ctx = u->ctx;
    TSQ_HIP(&u->hdr, hipEventRecord(u->ev[1], ctx->stream));
    TSQ_HIP(&u->hdr, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, u->ev[0], u->ev[1]) == hipSuccess) u->kernel_ms += ms;
    return TSQ_OK;
}

// first byte and byte count of rows [cursor, cursor + n) of the var-len columns
tsq_status us_var_range(tsq_unionscan* u, int64_t n) {
    if (u->peek_cursor == u->cursor && u->peek_rows == n) return TSQ_OK;
    tsq_ctx* ctx = u->ctx;
    tsq_handle_hdr* h = &u->hdr;
    const int n_cols = u->cfg.n_cols;
    int slot = 0;
    for (int c = 0; c < n_cols; c++) {
        if (u->cfg.col_types[c] != TSQ_BYTES) continue;
        if (slot >= 4) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "more than 4 var-len columns in one union scan");
        const int64_t* qo = u->q_offs[c].as<int64_t>();
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 48 + 2 * slot, qo + u->cursor, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 49 + 2 * slot, qo + u->cursor + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        slot++;
    }
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    slot = 0;
    for (int c = 0; c < n_cols; c++) {
        u->vlo[c] = u->vbytes[c] = 0;
        if (u->cfg.col_types[c] != TSQ_BYTES) continue;
        u->vlo[c] = (int64_t)ctx->pinned[48 + 2 * slot];
        u->vbytes[c] = (int64_t)ctx->pinned[49 + 2 * slot] - u->vlo[c];
        slot++;
    }
    u->peek_cursor = u->cursor;
    u->peek_rows = n;
    return TSQ_OK;
}
}  // namespace

TSQ_API int64_t tsq_unionscan_set_slots(int64_t n_handles) { return n_handles <= 0 ? 0 : (int64_t)tsq_us_set_slots((uint64_t)n_handles); }

namespace {
// dev: the two handle arrays are device memory and the set is built by k_us_build
tsq_status us_create(tsq_ctx* ctx, const tsq_unionscan_cfg* cfg, const int64_t* added_handles, int64_t n_added, const int64_t* deleted_handles, int64_t n_deleted,
                     bool dev, tsq_unionscan** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !cfg || !out) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_unionscan_create: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (cfg->n_cols < 1 || cfg->n_cols > TSQ_MAX_COLS) return tsq_fail(ch, TSQ_ERR_INVALID, "union scan: 1..16 columns");
    if (cfg->n_keys < 0 || cfg->n_keys > TSQ_MAX_KEYS) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "union scan: 0..4 index columns supported");
    for (int c = 0; c < cfg->n_cols; c++)
        if (cfg->col_types[c] < TSQ_I64 || cfg->col_types[c] > TSQ_BYTES) return tsq_fail(ch, TSQ_ERR_INVALID, "unknown column type");
    for (int k = 0; k < cfg->n_keys; k++)
        if (cfg->key_col[k] < 0 || cfg->key_col[k] >= cfg->n_cols) return tsq_fail(ch, TSQ_ERR_INVALID, "union scan: index column out of range");
    if (cfg->handle_col < 0 || cfg->handle_col >= cfg->n_cols) return tsq_fail(ch, TSQ_ERR_INVALID, "union scan: handle column out of range");
    if (cfg->col_types[cfg->handle_col] != TSQ_I64 && cfg->col_types[cfg->handle_col] != TSQ_U64)
        return tsq_fail(ch, TSQ_ERR_INVALID, "union scan: the handle column must be an 8-byte integer column");
    if (n_added < 0 || n_deleted < 0 || (n_added > 0 && !added_handles) || (n_deleted > 0 && !deleted_handles))
        return tsq_fail(ch, TSQ_ERR_INVALID, "union scan: bad handle arrays");
    if (n_added + n_deleted >= (1LL << 31)) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "union scan: 2^31 dirty handles or more");
    std::unique_ptr<tsq_unionscan> u(new tsq_unionscan());
    u->hdr.magic = TSQ_MAGIC_UNIONSCAN;
    u->ctx = ctx;
    u->cfg = *cfg;
    memset(&u->order, 0, sizeof u->order);
    u->order.n_keys = cfg->n_keys;
    for (int k = 0; k < cfg->n_keys; k++) u->order.key_col[k] = cfg->key_col[k];
    u->order.handle_col = cfg->handle_col;
    u->order.desc = cfg->desc ? 1 : 0;
    const int nc = cfg->n_cols;
    u->added.resize(nc);
    u->snap.resize(nc);
    for (int c = 0; c < nc; c++) u->added[c].type = u->snap[c].type = cfg->col_types[c];
    u->q_data.resize(nc);
    u->q_nn.resize(nc);
    u->q_offs.resize(nc);
    u->q_bytes.assign(nc, 0);
    u->obm.resize(nc);
    u->ooffs.resize(nc);
    u->vlo.assign(nc, 0);
    u->vbytes.assign(nc, 0);
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    // the handle set: built here with the probe's own code (tsq_unionscan_dp.h), then copied to HBM once
    u->set_slots = tsq_us_set_slots((uint64_t)(n_added + n_deleted));
    tsq_status st = TSQ_OK;
    if (u->set_slots && dev) {
        st = u->set_keys.reserve(ctx, ch, (size_t)u->set_slots * 8);
        if (st == TSQ_OK) st = u->set_occ.reserve(ctx, ch, (size_t)(u->set_slots / 32) * 4);
        hipError_t e = hipSuccess;
        if (st == TSQ_OK) e = hipMemsetAsync(u->set_keys.p, 0, (size_t)u->set_slots * 8, ctx->stream);
        if (st == TSQ_OK && e == hipSuccess) e = hipMemsetAsync(u->set_occ.p, 0, (size_t)(u->set_slots / 32) * 4, ctx->stream);
        if (st == TSQ_OK && e == hipSuccess) {
            UsBuildArgs b;
            memset(&b, 0, sizeof b);
            b.added = added_handles, b.n_added = n_added, b.deleted = deleted_handles, b.n_deleted = n_deleted;
            b.keys = u->set_keys.as<uint64_t>(), b.occ = u->set_occ.as<uint32_t>(), b.slots = u->set_slots;
            hipLaunchKernelGGL(k_us_build, dim3(tsq_grid_for(ctx, n_added + n_deleted, 256)), dim3(256), 0, ctx->stream, b);
            e = hipGetLastError();
        }
        if (st == TSQ_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the caller's arrays are free again
        if (st == TSQ_OK && e != hipSuccess) st = tsq_fail(ch, TSQ_ERR_HIP, std::string("union scan: ") + hipGetErrorString(e));
    } else if (u->set_slots) {
        std::vector<uint64_t> keys((size_t)u->set_slots, 0);
        std::vector<uint32_t> occ((size_t)(u->set_slots / 32), 0);
        for (int64_t i = 0; i < n_added; i++) tsq_us_set_insert(keys.data(), occ.data(), u->set_slots, (uint64_t)added_handles[i]);
        for (int64_t i = 0; i < n_deleted; i++) tsq_us_set_insert(keys.data(), occ.data(), u->set_slots, (uint64_t)deleted_handles[i]);
        st = u->set_keys.reserve(ctx, ch, keys.size() * 8);
        if (st == TSQ_OK) st = u->set_occ.reserve(ctx, ch, occ.size() * 4);
        hipError_t e = hipSuccess;
        if (st == TSQ_OK) e = hipMemcpyAsync(u->set_keys.p, keys.data(), keys.size() * 8, hipMemcpyHostToDevice, ctx->stream);
        if (st == TSQ_OK && e == hipSuccess) e = hipMemcpyAsync(u->set_occ.p, occ.data(), occ.size() * 4, hipMemcpyHostToDevice, ctx->stream);
        if (st == TSQ_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);  // the vectors go away
        if (st == TSQ_OK && e != hipSuccess) st = tsq_fail(ch, TSQ_ERR_HIP, std::string("union scan: ") + hipGetErrorString(e));
    }
    for (int i = 0; i < 2 && st == TSQ_OK; i++)
        if (u->ev[i].create() != hipSuccess) st = tsq_fail(ch, TSQ_ERR_HIP, "hipEventCreate");
    if (st != TSQ_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return st;
    }
    *out = u.release();
    return TSQ_OK;
}
}  // namespace

TSQ_API tsq_status tsq_unionscan_create(tsq_ctx* ctx, const tsq_unionscan_cfg* cfg, const int64_t* added_handles, int64_t n_added,
                                        const int64_t* deleted_handles, int64_t n_deleted, tsq_unionscan** out) {
    return us_create(ctx, cfg, added_handles, n_added, deleted_handles, n_deleted, false, out);
}
TSQ_API tsq_status tsq_unionscan_create_dev(tsq_ctx* ctx, const tsq_unionscan_cfg* cfg, const int64_t* added_handles, int64_t n_added,
                                            const int64_t* deleted_handles, int64_t n_deleted, tsq_unionscan** out) {
    return us_create(ctx, cfg, added_handles, n_added, deleted_handles, n_deleted, true, out);
}

TSQ_API tsq_status tsq_unionscan_set_added(tsq_unionscan* u, const tsq_col* cols, int32_t n_cols, int64_t nrows) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(u, TSQ_MAGIC_UNIONSCAN));
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return TSQ_ERR_INVALID;
    TSQ_TRY(us_cancelled(u));
    tsq_handle_hdr* h = &u->hdr;
    if (u->added_set) return tsq_fail(h, TSQ_ERR_INVALID, "set_added: the added rows were already set");
    if (u->pushed) return tsq_fail(h, TSQ_ERR_INVALID, "set_added after a push");
    if (u->finished) return tsq_fail(h, TSQ_ERR_INVALID, "set_added after finish");
    if (nrows < 0 || (!cols && nrows > 0)) return tsq_fail(h, TSQ_ERR_INVALID, "bad arguments");
    if (nrows >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "union scan: 2^31 added rows or more");
    u->added_set = true;
    if (nrows == 0) return TSQ_OK;
    bool dev = false;
    TSQ_TRY(tsq_validate_cols(h, cols, n_cols, u->cfg.n_cols, u->cfg.col_types, nrows, &dev));
    tsq_ctx* ctx = u->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    for (int c = 0; c < n_cols; c++) {
        TSQ_TRY(cols[c].type == TSQ_BYTES
                    ? tsq_col_append_varlen(ctx, h, u->added[c], cols[c].data, cols[c].offsets, cols[c].null_bitmap, nrows, dev, u->tmp_bits, u->tmp_offs)
                    : tsq_col_append(ctx, h, u->added[c], cols[c].data, cols[c].null_bitmap, nrows, dev, u->tmp_bits));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // the staging buffers are reused by the next column
    }
    u->n_added = nrows;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionscan_push(tsq_unionscan* u, const tsq_col* cols, int32_t n_cols, int64_t nrows) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(u, TSQ_MAGIC_UNIONSCAN));
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return TSQ_ERR_INVALID;
    TSQ_TRY(us_cancelled(u));
    tsq_handle_hdr* h = &u->hdr;
    tsq_ctx* ctx = u->ctx;
    if (u->finished) return tsq_fail(h, TSQ_ERR_INVALID, "push after finish");
    if (nrows < 0 || (!cols && nrows > 0)) return tsq_fail(h, TSQ_ERR_INVALID, "bad arguments");
    if (nrows >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "union scan: 2^31 rows or more in one push");
    u->pushed = true;
    if (nrows == 0) return TSQ_OK;
    bool dev = false;
    TSQ_TRY(tsq_validate_cols(h, cols, n_cols, u->cfg.n_cols, u->cfg.col_types, nrows, &dev));
    TSQ_HIP(h, hipSetDevice(ctx->device));
    tsq_us_run S;
    memset(&S, 0, sizeof S);
    if (dev) {
        tsq_colset_from_cols(S.cs, cols, n_cols);  // read in place: every kernel of this push has ended when the call returns
    } else {
        for (int c = 0; c < n_cols; c++) {
            u->snap[c].clear();
            TSQ_TRY(cols[c].type == TSQ_BYTES
                        ? tsq_col_append_varlen(ctx, h, u->snap[c], cols[c].data, cols[c].offsets, cols[c].null_bitmap, nrows, false, u->tmp_bits, u->tmp_offs)
                        : tsq_col_append(ctx, h, u->snap[c], cols[c].data, cols[c].null_bitmap, nrows, false, u->tmp_bits));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        }
        tsq_fill_colset(S.cs, u->snap);
    }
    S.v.n = nrows;
    TSQ_HIP(h, hipEventRecord(u->ev[0], ctx->stream));
    // ---- the filter: kept-row list + its length
    int64_t n_kept = nrows;
    UsMergeArgs b;
    memset(&b, 0, sizeof b);
    if (u->set_slots) {
        UsFilterArgs f;
        memset(&f, 0, sizeof f);
        f.handles = (const int64_t*)S.cs.data[u->cfg.handle_col];
        f.nrows = nrows;
        f.set.keys = u->set_keys.as<uint64_t>();
        f.set.occ = u->set_occ.as<uint32_t>();
        f.set.slots = u->set_slots;
        const int grid = tsq_grid_for(ctx, nrows, 256);
        const int n_runs = grid * 4;
        f.rows_per_wave = (((nrows + n_runs - 1) / n_runs) + 63) & ~(int64_t)63;
        TSQ_TRY(u->keep.reserve(ctx, h, (size_t)nrows + 64));
        TSQ_TRY(u->kept_rows.reserve(ctx, h, (size_t)nrows * 4 + 64));
        TSQ_TRY(u->base.reserve(ctx, h, (size_t)n_runs * 8 + 64));
        f.keep = u->keep.as<uint8_t>();
        f.kept_rows = u->kept_rows.as<uint32_t>();
        f.block_base = u->base.as<unsigned long long>();
        f.total = f.block_base + n_runs;
        hipLaunchKernelGGL(k_us_probe, dim3(grid), dim3(256), 0, ctx->stream, f);
        hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, f.block_base, n_runs, f.total);
        hipLaunchKernelGGL(k_us_scatter, dim3(grid), dim3(256), 0, ctx->stream, f);
        TSQ_HIP(h, hipGetLastError());
        S.v.rows = f.kept_rows;
        b.n_kept = f.total;
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 44, f.total, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    // ---- the streaming rule's m: added rows from the cursor that precede the last kept row
    int64_t m = 0;
    const int64_t a_left = u->n_added - u->a_cursor;
    if (a_left > 0) {
        b.order = u->order;
        b.S = S;
        us_fill_run(b.A, u->added);
        b.A.v.base = u->a_cursor;
        b.A.v.n = a_left;
        b.m_out = (unsigned long long*)ctx->dscratch + 8;
        hipLaunchKernelGGL(k_us_bound, dim3(1), dim3(64), 0, ctx->stream, b);
        TSQ_HIP(h, hipGetLastError());
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 45, b.m_out, 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    if (u->set_slots || a_left > 0) {
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        if (u->set_slots) n_kept = std::min<int64_t>(nrows, (int64_t)ctx->pinned[44]);
        if (a_left > 0) m = std::min<int64_t>(a_left, (int64_t)ctx->pinned[45]);
    }
    u->snapshot_rows += nrows;
    u->dropped_rows += nrows - n_kept;
    if (n_kept == 0) m = 0;  // S did not grow: nothing becomes determined
    TSQ_TRY(us_merge_emit(u, S, nrows, n_kept, m));
    return us_timed_end(u);
}

TSQ_API tsq_status tsq_unionscan_finish(tsq_unionscan* u) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(u, TSQ_MAGIC_UNIONSCAN));
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return TSQ_ERR_INVALID;
    TSQ_TRY(us_cancelled(u));
    if (u->finished) return TSQ_OK;
    u->finished = true;
    const int64_t m = u->n_added - u->a_cursor;
    if (m <= 0) return TSQ_OK;
    TSQ_HIP(&u->hdr, hipSetDevice(u->ctx->device));
    TSQ_HIP(&u->hdr, hipEventRecord(u->ev[0], u->ctx->stream));
    tsq_us_run S;  // no snapshot rows: the rest of the added rows
    memset(&S, 0, sizeof S);
    TSQ_TRY(us_merge_emit(u, S, 0, 0, m));
    return us_timed_end(u);
}

TSQ_API tsq_status tsq_unionscan_peek(tsq_unionscan* u, int64_t cap_rows, int64_t* nrows_out, int64_t* bytes_out, int32_t n_cols) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(u, TSQ_MAGIC_UNIONSCAN));
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return TSQ_ERR_INVALID;
    if (!nrows_out || !bytes_out) return tsq_fail(&u->hdr, TSQ_ERR_INVALID, "NULL out pointer");
    *nrows_out = 0;
    TSQ_TRY(us_cancelled(u));
    if (n_cols != u->cfg.n_cols) return tsq_fail(&u->hdr, TSQ_ERR_INVALID, "peek: column count must equal the input schema");
    for (int c = 0; c < n_cols; c++) bytes_out[c] = 0;
    const int64_t n = std::min<int64_t>(cap_rows, u->q_rows - u->cursor);
    if (n <= 0) return TSQ_OK;
    bool any_var = false;
    for (int c = 0; c < n_cols; c++) any_var = any_var || u->cfg.col_types[c] == TSQ_BYTES;
    if (any_var) {
        TSQ_HIP(&u->hdr, hipSetDevice(u->ctx->device));
        TSQ_TRY(us_var_range(u, n));
        for (int c = 0; c < n_cols; c++) bytes_out[c] = u->vbytes[c];
    }
    *nrows_out = n;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionscan_pull(tsq_unionscan* u, tsq_col* out_cols, int32_t n_cols, int64_t cap_rows, int64_t* nrows_out, int32_t* eos) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(u, TSQ_MAGIC_UNIONSCAN));
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &u->hdr;
    if (!nrows_out || !eos) return tsq_fail(h, TSQ_ERR_INVALID, "NULL out pointer");
    *nrows_out = 0;
    *eos = 0;
    TSQ_TRY(us_cancelled(u));
    if (n_cols != u->cfg.n_cols) return tsq_fail(h, TSQ_ERR_INVALID, "pull: column count must equal the input schema");
    const int64_t n = std::min<int64_t>(cap_rows, u->q_rows - u->cursor);
    if (n <= 0) {
        *eos = u->finished ? 1 : 0;
        return TSQ_OK;
    }
    if (!out_cols) return tsq_fail(h, TSQ_ERR_INVALID, "pull: out_cols == NULL");
    tsq_ctx* ctx = u->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool odev = out_cols[0].flags & TSQ_COL_DEVICE;
    bool any_var = false;
    for (int c = 0; c < n_cols; c++) {
        const bool var = u->cfg.col_types[c] == TSQ_BYTES;
        any_var = any_var || var;
        if (!out_cols[c].null_bitmap || (var ? !out_cols[c].offsets : !out_cols[c].data))
            return tsq_fail(h, TSQ_ERR_INVALID, "pull: out columns need data and null_bitmap buffers (a var-len column: offsets, and data for the bytes tsq_unionscan_peek announced)");
        if (((out_cols[c].flags & TSQ_COL_DEVICE) != 0) != odev) return tsq_fail(h, TSQ_ERR_INVALID, "pull: mixed host/device outputs");
    }
    if (any_var) TSQ_TRY(us_var_range(u, n));
    const hipMemcpyKind kind = odev ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    for (int c = 0; c < n_cols; c++) {
        const bool var = u->cfg.col_types[c] == TSQ_BYTES;
        const int es = var ? 0 : tsq_elem_size(u->cfg.col_types[c]);
        // the NOT-NULL flags of the queue -> the packed bitmap
        uint8_t* bm = out_cols[c].null_bitmap;
        if (!odev) {
            TSQ_TRY(u->obm[c].reserve(ctx, h, tsq_bitmap_bytes(n) + 64));
            bm = u->obm[c].as<uint8_t>();
        }
        TSQ_TRY(tsq_launch_pack_bitmap(ctx, h, u->q_nn[c].as<uint8_t>() + u->cursor, bm, n));
        if (!odev) TSQ_HIP(h, hipMemcpyAsync(out_cols[c].null_bitmap, bm, tsq_bitmap_bytes(n), hipMemcpyDeviceToHost, ctx->stream));
        if (!var) {
            TSQ_HIP(h, hipMemcpyAsync(out_cols[c].data, (const char*)u->q_data[c].p + (size_t)u->cursor * es, (size_t)n * es, kind, ctx->stream));
        } else {
            const int64_t nbytes = u->vbytes[c];
            if (nbytes > 0 && !out_cols[c].data) return tsq_fail(h, TSQ_ERR_INVALID, "pull: a var-len column needs a data buffer (tsq_unionscan_peek tells its size)");
            int64_t* offs = out_cols[c].offsets;
            if (!odev) {
                TSQ_TRY(u->ooffs[c].reserve(ctx, h, ((size_t)n + 1) * 8 + 64));
                offs = u->ooffs[c].as<int64_t>();
            }
            TSQ_TRY(tsq_launch_offsets_rebase(ctx, h, offs, u->q_offs[c].as<int64_t>() + u->cursor, n + 1, -u->vlo[c]));
            if (!odev) TSQ_HIP(h, hipMemcpyAsync(out_cols[c].offsets, offs, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (nbytes > 0) TSQ_HIP(h, hipMemcpyAsync(out_cols[c].data, u->q_data[c].as<uint8_t>() + u->vlo[c], (size_t)nbytes, kind, ctx->stream));
        }
    }
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    u->peek_cursor = -1;
    for (int c = 0; c < n_cols; c++) {
        const bool var = u->cfg.col_types[c] == TSQ_BYTES;
        out_cols[c].length = n;
        out_cols[c].type = u->cfg.col_types[c];
        out_cols[c].elem_size = var ? -1 : tsq_elem_size(u->cfg.col_types[c]);
    }
    u->cursor += n;
    *nrows_out = n;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionscan_stats(tsq_unionscan* u, int64_t* snapshot_rows, int64_t* dropped_rows, int64_t* added_rows_out, double* kernel_ms) {
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return TSQ_ERR_INVALID;
    if (snapshot_rows) *snapshot_rows = u->snapshot_rows;
    if (dropped_rows) *dropped_rows = u->dropped_rows;
    if (added_rows_out) *added_rows_out = u->added_out;
    if (kernel_ms) *kernel_ms = u->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionscan_cancel(tsq_unionscan* u) {
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return TSQ_ERR_INVALID;
    u->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_unionscan_destroy(tsq_unionscan* u) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(u, TSQ_MAGIC_UNIONSCAN));
    if (!u || u->hdr.magic != TSQ_MAGIC_UNIONSCAN) return;
    (void)hipSetDevice(u->ctx->device);
    (void)hipStreamSynchronize(u->ctx->stream);
    u->hdr.magic = 0;
    delete u;
}
