// tsq_groupid.hip — a dictionary of GROUP KEYS over 1..16 key columns (tsq_groupid_*): rows -> dense 32-bit group ids in order of first
// occurrence, and the distinct key rows as ordinary chunk-layout columns.  It is the front of GROUP BY / SELECT DISTINCT over more than
// TSQ_MAX_GROUP_KEYS columns (tsq_agg_create_keys: the ids feed a one-key aggregate), whose four-key routes keep their key words in
// registers and are not widened.
//
// The table is open addressing in HBM over 64-bit slots (tsq_groupid_dp.h: tag | id), at most half full.  A call is worked through in
// SLICES of at most 2^22 rows; per slice (G = groups before it):
//   K14a k_gid_claim   : a row hashes its N cell images and walks the table.  Empty slot: claimed with one CAS, value G + row.  Tag match
//                        with a value < G (a key of an earlier slice / call): the row's cells are compared with the DICTIONARY row; equal ->
//                        the id is final.  Tag match with a value >= G (a key this slice brought): the cells are compared with the INPUT row
//                        value - G — the slot's current representative; equal -> atomicMin(slot, G + row).  Every row that ever wins a slot
//                        holds the key of its first claimant, so the comparison is exact whichever representative it meets.  Unequal -> the
//                        walk goes on (counted: collision_rows).  The row leaves its slot number in ids_out.
//   K14b k_gid_flag    : a row is the FIRST row of a new group iff its slot holds G + row (the minimum of its claimants)
//        k_compact_count / k_compact_scan (tsq_compact.h): rank of every first row, in row order
//   K14c k_gid_bind    : first rows write id = G + rank into their slot and the row hash beside the dictionary (growth reads no key)
//        tsq_chunk_compact + ColStore appends: the first rows' key cells become dictionary rows G.. (var-len columns and bitmaps included)
//   K14d k_gid_resolve : every other row reads the id from its slot
// No wave ever waits for a store of another wave: kernel boundaries on the context's stream are the only synchronisation, every walk is
// bounded by the table size.  Ids are deterministic — first occurrence in row order within a call, call order across calls — whatever
// the interleaving, and an id once given never changes.
// Between slices: the cancel flag; when the next slice could fill the table beyond one half, a table twice as large is filled from the
// stored (hash, id) pairs (k_gid_rehash).
// Algorithmic bytes per row: K14a reads N x 8 B of keys (+ the cells of the rows it is compared with, L2 resident for few groups) and
// writes 8 B; K14b reads 8 B + the slot, writes 1 B; K14d reads 8 B + the slot, writes 8 B of id.
#include "tsq_stage.h"
#include "tsq_compact.h"
#include "tsq_groupid_dp.h"

#include <memory>

#define GID_PROV 0x8000000000000000ULL  /* ids_out while a slice is in flight: this bit | the row's slot number */
#define GID_SLICE_ROWS ((int64_t)1 << 22)
#define GID_MIN_ROOM 4096
#define GID_MAX_SLOTS ((uint64_t)1 << 32)

struct GidArgs {
    tsq_colset in;    // the slice's key columns
    tsq_colset dict;  // the dictionary columns (rows [0, base))
    unsigned long long* tab;
    uint64_t cap_mask;
    uint64_t hash_mask;  // ~0, or (tests) the low TSQ_KNOB_GROUPID_TAG_BITS bits
    uint32_t base;       // groups before this slice
    int64_t nrows;
    uint64_t* ids;
    uint8_t* flags;
    unsigned long long* counters;  // [0] rows that walked past a slot with their tag after a comparison (cumulative) [1] walks that found no slot
    int64_t rows_per_wave;         // K14c: the runs of k_compact_count
    const unsigned long long* wave_base;
    uint64_t* dict_hash;
};

__global__ void __launch_bounds__(256) k_gid_claim(GidArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    unsigned int n_coll = 0, n_lost = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nrows; r += stride) {
        const uint64_t h = gid_row_hash(a.in, r) & a.hash_mask;
        const uint64_t tag = gid_slot_tag(h);
        const unsigned long long mine = tag | (uint64_t)(a.base + (uint32_t)r);
        uint64_t idx = h & a.cap_mask, out = ~0ull;
        bool collided = false;
        for (uint64_t step = 0; step <= a.cap_mask; step++) {  // (the table is at most half full: an empty slot ends the walk long before)
            unsigned long long s = __hip_atomic_load(&a.tab[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s == 0) {
                s = atomicCAS(&a.tab[idx], 0ull, mine);
                if (s == 0) {
                    out = GID_PROV | idx;
                    break;
                }
            }
            if ((s & 0xffffffff00000000ULL) == tag) {
                const uint32_t v = (uint32_t)s;
                if (v < a.base) {
                    if (gid_rows_equal(a.in, r, a.dict, (int64_t)v)) {
                        out = v;
                        break;
                    }
                } else if (gid_rows_equal(a.in, r, a.in, (int64_t)(v - a.base))) {
                    atomicMin(&a.tab[idx], mine);
                    out = GID_PROV | idx;
                    break;
                }
                collided = true;
            }
            idx = (idx + 1) & a.cap_mask;
        }
        a.ids[r] = out;
        n_coll += collided ? 1u : 0u;
        n_lost += out == ~0ull ? 1u : 0u;
    }
    for (int o = 32; o > 0; o >>= 1) {
        n_coll += __shfl_xor(n_coll, o, 64);
        n_lost += __shfl_xor(n_lost, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (n_coll) atomicAdd(&a.counters[0], (unsigned long long)n_coll);
        if (n_lost) atomicAdd(&a.counters[1], (unsigned long long)n_lost);
    }
}

__global__ void __launch_bounds__(256) k_gid_flag(GidArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nrows; r += stride) {
        const uint64_t w = a.ids[r];
        uint8_t first = 0;
        if (w != ~0ull && (w & GID_PROV)) first = (uint32_t)a.tab[w & ~GID_PROV] == a.base + (uint32_t)r ? 1 : 0;
        a.flags[r] = first;
    }
}

// the runs and the walk of k_compact_scatter (tsq_chunk.hip): dense position = rank among the first rows, in row order
__global__ void __launch_bounds__(256) k_gid_bind(GidArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = u * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.nrows ? hi : a.nrows;
    unsigned long long cur = lo < a.nrows ? a.wave_base[u] : 0ull;
    for (int64_t r = lo + lane; r - lane < hi; r += 64) {
        const bool sel = r < hi && a.flags[r];
        const unsigned long long m = __ballot(sel);
        const unsigned long long pos = cur + __popcll(m & ((1ull << lane) - 1ull));
        cur += (unsigned long long)__popcll(m);
        if (!sel) continue;
        const uint64_t slot = a.ids[r] & ~GID_PROV;
        const uint64_t id = (uint64_t)a.base + pos;
        a.tab[slot] = (a.tab[slot] & 0xffffffff00000000ULL) | id;  // (this row is the slot's only writer in this kernel)
        a.dict_hash[id] = gid_row_hash(a.in, r);
    }
}

__global__ void __launch_bounds__(256) k_gid_resolve(GidArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nrows; r += stride) {
        const uint64_t w = a.ids[r];
        if (w != ~0ull && (w & GID_PROV)) a.ids[r] = (uint32_t)a.tab[w & ~GID_PROV];
    }
}

// growth: the (hash, id) pairs of all groups into an empty table twice as large; the keys are distinct, no cell is read
__global__ void __launch_bounds__(256) k_gid_rehash(unsigned long long* tab, uint64_t cap_mask, uint64_t hash_mask, const uint64_t* dict_hash, int64_t n_groups,
                                                    unsigned long long* counters) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t g = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; g < n_groups; g += stride) {
        const uint64_t h = dict_hash[g] & hash_mask;
        const unsigned long long mine = gid_slot_tag(h) | (uint64_t)g;
        uint64_t idx = h & cap_mask;
        bool placed = false;
        for (uint64_t step = 0; step <= cap_mask && !placed; step++) {
            placed = atomicCAS(&tab[idx], 0ull, mine) == 0;
            idx = (idx + 1) & cap_mask;
        }
        if (!placed) atomicAdd(&counters[1], 1ull);
    }
}

struct tsq_groupid {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    int32_t n_keys = 0;
    int32_t types[TSQ_GROUPID_MAX_KEYS];
    std::atomic<int> cancelled{0};
    DevBuf tab;
    uint64_t cap = 0;
    uint64_t hash_mask = ~0ull;
    int64_t groups = 0;
    std::vector<ColStore> dict;  // one column per key, row g = the key cells of the first row of group g
    DevBuf dict_hash, flags, base, counters;
    DevBuf tdata[TSQ_GROUPID_MAX_KEYS], tbm[TSQ_GROUPID_MAX_KEYS], toffs[TSQ_GROUPID_MAX_KEYS], tmp_bits, tmp_offs;  // a slice's new key rows on their way
    DevEvent ev0, ev1;
    int64_t rows = 0, collision_rows = 0;
    int32_t rehashes = 0;
    double kernel_ms = 0;
};

namespace {

tsq_status gid_cancelled(tsq_groupid* g) {
    if (g->cancelled.load()) return tsq_fail(&g->hdr, TSQ_ERR_CANCELLED, "group-id dictionary cancelled");
    return TSQ_OK;
}

tsq_status gid_new_table(tsq_groupid* g, uint64_t cap, DevBuf& t) {
    TSQ_TRY(t.reserve(g->ctx, &g->hdr, (size_t)cap * 8));
    TSQ_HIP(&g->hdr, hipMemsetAsync(t.p, 0, (size_t)cap * 8, g->ctx->stream));
    return TSQ_OK;
}

tsq_status gid_grow(tsq_groupid* g, uint64_t new_cap) {
    tsq_ctx* ctx = g->ctx;
    DevBuf nt;
    tsq_status s = gid_new_table(g, new_cap, nt);
    if (s == TSQ_OK && g->groups > 0) {
        hipLaunchKernelGGL(k_gid_rehash, dim3(tsq_grid_for(ctx, g->groups, 256)), dim3(256), 0, ctx->stream, nt.as<unsigned long long>(), new_cap - 1, g->hash_mask,
                           g->dict_hash.as<uint64_t>(), g->groups, g->counters.as<unsigned long long>());
        const hipError_t e = hipGetLastError();
        if (e != hipSuccess) s = tsq_fail(&g->hdr, TSQ_ERR_HIP, hipGetErrorString(e));
    }
    TSQ_TRY(s);
    g->tab = std::move(nt);  // (stream order protects the old table: DevBuf's pool rule)
    g->cap = new_cap;
    g->rehashes++;
    return TSQ_OK;
}

void gid_fill_dict(const tsq_groupid* g, tsq_colset& d) { tsq_fill_colset(d, g->dict); }

// rows [off, off + n) of the caller's key columns (off: a multiple of 8)
void gid_slice_cols(const tsq_col* in, int32_t n_keys, int64_t off, int64_t n, tsq_col* out) {
    for (int c = 0; c < n_keys; c++) {
        out[c] = in[c];
        if (in[c].type == TSQ_BYTES) out[c].offsets = in[c].offsets + off;
        else out[c].data = (char*)in[c].data + (size_t)off * tsq_elem_size(in[c].type);
        if (in[c].null_bitmap) out[c].null_bitmap = in[c].null_bitmap + (off >> 3);
        out[c].length = n;
    }
}

// the key cells of the slice's n_new first rows -> dictionary rows [groups, groups + n_new)
tsq_status gid_append_keys(tsq_groupid* g, const tsq_col* cols, int64_t n, int64_t n_new) {
    tsq_ctx* ctx = g->ctx;
    tsq_handle_hdr* h = &g->hdr;
    tsq_col out[TSQ_GROUPID_MAX_KEYS];
    for (int c = 0; c < g->n_keys; c++) {
        out[c] = cols[c];
        out[c].flags = TSQ_COL_DEVICE;
        if (cols[c].type == TSQ_BYTES) {  // a selection never grows: the slice's bytes bound the new rows' bytes
            TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 20, cols[c].offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 21, cols[c].offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
            const int64_t bytes = (int64_t)ctx->pinned[21] - (int64_t)ctx->pinned[20];
            if (bytes < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_groupid_assign: var-len key column: offsets must not decrease");
            TSQ_TRY(g->tdata[c].reserve(ctx, h, (size_t)bytes + 64));
            TSQ_TRY(g->toffs[c].reserve(ctx, h, ((size_t)n_new + 2) * 8 + 64));
            out[c].offsets = g->toffs[c].as<int64_t>();
        } else {
            TSQ_TRY(g->tdata[c].reserve(ctx, h, (size_t)n_new * 8 + 64));
        }
        out[c].data = g->tdata[c].p;
        out[c].null_bitmap = nullptr;
        if (cols[c].null_bitmap) {
            TSQ_TRY(g->tbm[c].reserve(ctx, h, tsq_bitmap_bytes(n_new) + 64));
            out[c].null_bitmap = g->tbm[c].as<uint8_t>();
        }
    }
    int64_t n_out = 0;
    const tsq_status cs = tsq_chunk_compact(ctx, cols, g->n_keys, n, g->flags.as<uint8_t>(), out, &n_out);
    if (cs != TSQ_OK) return tsq_fail(h, cs, "tsq_groupid_assign: " + ctx->hdr.err);
    if (n_out != n_new) return tsq_fail(h, TSQ_ERR_HIP, "tsq_groupid_assign: the compaction kept another number of rows than the positions pass counted");
    for (int c = 0; c < g->n_keys; c++) {
        if (cols[c].type == TSQ_BYTES) TSQ_TRY(tsq_col_append_varlen(ctx, h, g->dict[c], out[c].data, out[c].offsets, out[c].null_bitmap, n_new, true, g->tmp_bits, g->tmp_offs));
        else TSQ_TRY(tsq_col_append(ctx, h, g->dict[c], out[c].data, out[c].null_bitmap, n_new, true, g->tmp_bits));
    }
    return TSQ_OK;
}

tsq_status gid_slice(tsq_groupid* g, const tsq_col* cols, int64_t n, uint64_t* ids) {
    tsq_ctx* ctx = g->ctx;
    tsq_handle_hdr* h = &g->hdr;
    GidArgs a;
    memset(&a, 0, sizeof a);
    tsq_colset_from_cols(a.in, cols, g->n_keys);
    gid_fill_dict(g, a.dict);
    a.tab = g->tab.as<unsigned long long>();
    a.cap_mask = g->cap - 1;
    a.hash_mask = g->hash_mask;
    a.base = (uint32_t)g->groups;
    a.nrows = n;
    a.ids = ids;
    TSQ_TRY(g->flags.reserve(ctx, h, (size_t)n + 64));
    a.flags = g->flags.as<uint8_t>();
    a.counters = g->counters.as<unsigned long long>();
    const int grid = tsq_grid_for(ctx, n, 256);
    const int n_runs = grid * 4;
    CompactArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.selected = a.flags;
    ca.nrows = n;
    ca.rows_per_wave = (((n + n_runs - 1) / n_runs) + 63) & ~(int64_t)63;
    TSQ_TRY(g->base.reserve(ctx, h, (size_t)n_runs * 8 + 64));
    ca.block_base = g->base.as<unsigned long long>();
    ca.total = ca.block_base + n_runs;
    hipLaunchKernelGGL(k_gid_claim, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_gid_flag, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_compact_count, dim3(grid), dim3(256), 0, ctx->stream, ca);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, ca.block_base, n_runs, ca.total);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 16, ca.total, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 17, a.counters, 16, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t n_new = (int64_t)ctx->pinned[16];
    g->collision_rows = (int64_t)ctx->pinned[17];
    if (ctx->pinned[18] != 0) return tsq_fail(h, TSQ_ERR_HIP, "tsq_groupid_assign: a walk through the table found no slot");
    if (n_new < 0 || n_new > n) return tsq_fail(h, TSQ_ERR_HIP, "tsq_groupid_assign: the positions pass counted more rows than the slice has");
    if (n_new > 0) {
        TSQ_TRY(g->dict_hash.reserve(ctx, h, (size_t)(g->groups + n_new) * 8 + 64, true, (size_t)g->groups * 8));
        a.rows_per_wave = ca.rows_per_wave;
        a.wave_base = ca.block_base;
        a.dict_hash = g->dict_hash.as<uint64_t>();
        hipLaunchKernelGGL(k_gid_bind, dim3(grid), dim3(256), 0, ctx->stream, a);
        TSQ_HIP(h, hipGetLastError());
    }
    hipLaunchKernelGGL(k_gid_resolve, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    if (n_new > 0) TSQ_TRY(gid_append_keys(g, cols, n, n_new));
    g->groups += n_new;
    return TSQ_OK;
}

}  // namespace

TSQ_API tsq_status tsq_groupid_create(tsq_ctx* ctx, const int32_t* key_types, int32_t n_keys, int64_t est_groups, tsq_groupid** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || ctx->hdr.magic != TSQ_MAGIC_CTX || !out)
        return tsq_fail(ctx && ctx->hdr.magic == TSQ_MAGIC_CTX ? &ctx->hdr : nullptr, TSQ_ERR_INVALID, "tsq_groupid_create: bad arguments");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (n_keys < 1 || !key_types) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_groupid_create: n_keys must be at least 1");
    if (n_keys > TSQ_GROUPID_MAX_KEYS) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "tsq_groupid_create: 1..16 key columns supported");
    for (int k = 0; k < n_keys; k++)
        if (key_types[k] < TSQ_I64 || key_types[k] > TSQ_BYTES) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_groupid_create: unknown key column type");
    if (est_groups < 0) est_groups = 0;
    if ((uint64_t)est_groups >= GID_MAX_SLOTS / 2) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "tsq_groupid_create: fewer than 2^31 groups supported");
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    std::unique_ptr<tsq_groupid> g(new tsq_groupid());
    g->hdr.magic = TSQ_MAGIC_GROUPID;
    g->ctx = ctx;
    g->n_keys = n_keys;
    g->dict.resize(n_keys);
    for (int k = 0; k < n_keys; k++) g->types[k] = g->dict[k].type = key_types[k];
    const int64_t tb = tsq_knob(ctx, TSQ_KNOB_GROUPID_TAG_BITS, 0);
    if (tb > 0 && tb < 64) g->hash_mask = (1ull << tb) - 1ull;
    uint64_t cap = 2 * GID_MIN_ROOM;
    while (cap < (uint64_t)est_groups * 2 + 2 * GID_MIN_ROOM) cap <<= 1;
    tsq_status s = g->counters.reserve(ctx, &g->hdr, 64);
    if (s == TSQ_OK) s = gid_new_table(g.get(), cap, g->tab);
    if (s == TSQ_OK) {
        g->cap = cap;
        hipError_t e = hipMemsetAsync(g->counters.p, 0, 64, ctx->stream);
        if (e == hipSuccess) e = g->ev0.create();
        if (e == hipSuccess) e = g->ev1.create();
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e != hipSuccess) s = tsq_fail(&g->hdr, TSQ_ERR_HIP, hipGetErrorString(e));
    }
    if (s != TSQ_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return tsq_fail(ch, s, g->hdr.err);
    }
    *out = g.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_groupid_assign(tsq_groupid* g, const tsq_col* key_cols, int32_t n_keys, int64_t nrows, uint64_t* ids_out) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(g, TSQ_MAGIC_GROUPID));
    if (!g || g->hdr.magic != TSQ_MAGIC_GROUPID) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &g->hdr;
    TSQ_TRY(gid_cancelled(g));
    if (n_keys != g->n_keys || nrows < 0 || (nrows > 0 && (!key_cols || !ids_out))) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_groupid_assign: bad arguments");
    if (nrows >= ((int64_t)1 << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_groupid_assign: fewer than 2^31 rows per call supported");
    if (nrows == 0) return TSQ_OK;
    for (int c = 0; c < n_keys; c++) {
        if (!(key_cols[c].flags & TSQ_COL_DEVICE)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_groupid_assign: the key columns must be device resident (TSQ_COL_DEVICE)");
        if (key_cols[c].type != g->types[c]) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_groupid_assign: column type does not match the handle's key types");
        if (key_cols[c].length < nrows) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_groupid_assign: column shorter than nrows");
        if (key_cols[c].type == TSQ_BYTES ? !key_cols[c].offsets : !key_cols[c].data)
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_groupid_assign: column without data (or a var-len column without offsets)");
    }
    tsq_ctx* ctx = g->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    TSQ_HIP(h, hipEventRecord(g->ev0, ctx->stream));
    for (int64_t off = 0; off < nrows;) {
        TSQ_TRY(gid_cancelled(g));
        const int64_t want = std::min<int64_t>(nrows - off, GID_SLICE_ROWS);
        // every row of a slice may bring a key: the table holds at most cap / 2 groups after it
        if ((int64_t)(g->cap / 2) - g->groups < want) {
            uint64_t nc = g->cap * 2;
            while ((int64_t)(nc / 2) - g->groups < GID_MIN_ROOM) nc *= 2;
            if (nc > GID_MAX_SLOTS) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_groupid_assign: fewer than 2^31 groups supported");
            TSQ_TRY(gid_grow(g, nc));
        }
        int64_t n = std::min<int64_t>(want, (int64_t)(g->cap / 2) - g->groups);
        if (off + n < nrows) n &= ~(int64_t)63;  // (the next slice's null bitmaps start on a byte)
        tsq_col sl[TSQ_GROUPID_MAX_KEYS];
        gid_slice_cols(key_cols, n_keys, off, n, sl);
        TSQ_TRY(gid_slice(g, sl, n, ids_out + off));
        off += n;
    }
    TSQ_HIP(h, hipEventRecord(g->ev1, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, g->ev0, g->ev1) == hipSuccess) g->kernel_ms += ms;
    else (void)hipGetLastError();
    g->rows += nrows;
    return TSQ_OK;
}

// ---------------------------------------------------------------- FIRST_ROW(key column) of tsq_agg_create_keys from the dictionary
struct GidGatherArgs {
    const uint64_t* ids;
    int64_t n;
    const void* src;
    const uint8_t* src_nulls;
    const int64_t* src_offs;
    int32_t type;
    void* out;
    uint8_t* out_nn;
    int64_t* out_len;  // var-len: the cell lengths (a scan makes them offsets) and the cells' positions in the dictionary's bytes
    int64_t* out_pos;
};
__global__ void __launch_bounds__(256) k_gid_gather(GidGatherArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const int64_t g = (int64_t)a.ids[i];
        const bool null = tsq_is_null(a.src_nulls, g);
        a.out_nn[i] = null ? 0 : 1;
        if (a.type == TSQ_BYTES) {
            const int64_t o = a.src_offs[g];
            a.out_pos[i] = o;
            a.out_len[i] = null ? 0 : a.src_offs[g + 1] - o;
        } else if (a.type == TSQ_F32) {
            ((uint32_t*)a.out)[i] = ((const uint32_t*)a.src)[g];
        } else {
            ((uint64_t*)a.out)[i] = ((const uint64_t*)a.src)[g];
        }
    }
}

// ids[i] < the handle's groups (they are ids this handle gave); the caller holds the context lock
tsq_status tsq_groupid_gather_key(tsq_groupid* g, int32_t k, const uint64_t* ids, int64_t n, DevBuf& data, DevBuf& nn, DevBuf& offs, DevBuf& bytes, DevBuf& pos,
                                  DevBuf& scan_tmp, int64_t* nbytes) {
    tsq_ctx* ctx = g->ctx;
    tsq_handle_hdr* h = &g->hdr;
    *nbytes = 0;
    if (k < 0 || k >= g->n_keys || n < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_groupid_gather_key: bad arguments");
    if (n == 0) return TSQ_OK;
    const ColStore& d = g->dict[k];
    const bool str = d.type == TSQ_BYTES;
    GidGatherArgs a;
    memset(&a, 0, sizeof a);
    a.ids = ids;
    a.n = n;
    a.src = d.data.p;
    a.src_nulls = d.has_nulls ? d.nulls.as<uint8_t>() : nullptr;
    a.src_offs = str ? d.offs.as<int64_t>() : nullptr;
    a.type = d.type;
    TSQ_TRY(nn.reserve(ctx, h, (size_t)n + 64));
    a.out_nn = nn.as<uint8_t>();
    if (str) {
        TSQ_TRY(offs.reserve(ctx, h, ((size_t)n + 2) * 8 + 64));
        TSQ_TRY(pos.reserve(ctx, h, (size_t)n * 8 + 64));
        a.out_len = offs.as<int64_t>();
        a.out_pos = pos.as<int64_t>();
    } else {
        TSQ_TRY(data.reserve(ctx, h, (size_t)n * 8 + 64));
        a.out = data.p;
    }
    hipLaunchKernelGGL(k_gid_gather, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    if (!str) return TSQ_OK;
    TSQ_TRY(tsq_launch_scan64(ctx, h, offs.as<int64_t>(), n, scan_tmp));
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 22, offs.as<int64_t>() + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t total = (int64_t)ctx->pinned[22];
    TSQ_TRY(bytes.reserve(ctx, h, (size_t)total + 64));
    if (total > 0) TSQ_TRY(tsq_launch_var_copy(ctx, h, (const uint8_t*)d.data.p, pos.as<int64_t>(), offs.as<int64_t>(), n, total, bytes.as<uint8_t>()));
    *nbytes = total;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_groupid_count(tsq_groupid* g, int64_t* n_groups) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(g, TSQ_MAGIC_GROUPID));
    if (!g || g->hdr.magic != TSQ_MAGIC_GROUPID) return TSQ_ERR_INVALID;
    TSQ_TRY(gid_cancelled(g));
    if (!n_groups) return tsq_fail(&g->hdr, TSQ_ERR_INVALID, "tsq_groupid_count: NULL out pointer");
    *n_groups = g->groups;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_groupid_keys(tsq_groupid* g, tsq_col* out_cols, int32_t n_keys, int64_t* n_groups) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(g, TSQ_MAGIC_GROUPID));
    if (!g || g->hdr.magic != TSQ_MAGIC_GROUPID) return TSQ_ERR_INVALID;
    TSQ_TRY(gid_cancelled(g));
    if (!out_cols || !n_groups || n_keys != g->n_keys) return tsq_fail(&g->hdr, TSQ_ERR_INVALID, "tsq_groupid_keys: bad arguments");
    for (int c = 0; c < n_keys; c++) {
        const ColStore& d = g->dict[c];
        tsq_col& o = out_cols[c];
        memset(&o, 0, sizeof o);
        const bool str = d.type == TSQ_BYTES;
        o.type = d.type;
        o.data = d.data.p;
        o.null_bitmap = d.has_nulls ? d.nulls.as<uint8_t>() : nullptr;
        o.offsets = str ? d.offs.as<int64_t>() : nullptr;
        o.length = g->groups;
        o.elem_size = str ? -1 : tsq_elem_size(d.type);
        o.flags = TSQ_COL_DEVICE | TSQ_COL_BORROW;
    }
    *n_groups = g->groups;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_groupid_stats(tsq_groupid* g, int64_t* rows, int64_t* collision_rows, int32_t* rehashes, double* kernel_ms) {
    if (!g || g->hdr.magic != TSQ_MAGIC_GROUPID) return TSQ_ERR_INVALID;
    if (rows) *rows = g->rows;
    if (collision_rows) *collision_rows = g->collision_rows;
    if (rehashes) *rehashes = g->rehashes;
    if (kernel_ms) *kernel_ms = g->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_groupid_cancel(tsq_groupid* g) {
    if (!g || g->hdr.magic != TSQ_MAGIC_GROUPID) return TSQ_ERR_INVALID;
    g->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_groupid_destroy(tsq_groupid* g) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(g, TSQ_MAGIC_GROUPID));
    if (!g || g->hdr.magic != TSQ_MAGIC_GROUPID) return;
    (void)hipSetDevice(g->ctx->device);
    (void)hipStreamSynchronize(g->ctx->stream);
    g->hdr.magic = 0;
    delete g;
}
