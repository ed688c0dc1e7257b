// tsq_dupcheck.hip — the duplicate-key check of INSERT .. SELECT and the whole row logic of REPLACE .. SELECT on the GPU (gfx950):
// the statement's keys against the table's keys, against each other, and the outcome in the reference's row order
// (executor/insert.go:32-47, table/tables/tables.go:528-581, executor/replace.go:53-196, executor/batch_checker.go:66-157;
// include/tsq.h "Duplicate keys"; DESIGN.md §5 "Duplicate keys and REPLACE").
//
// A STREAM is one key that must be unique: the PK handle, or one unique index.  Per stream and statement row r:
//   ent_s[r]  : the store's entry with r's key, or -1        prev_s[r] : the latest earlier statement row with r's key, or -1
// tsq_dupcheck_create:
//        (HANDLE stream / table handles) tsq_lookup_create: the copy, the ascending check and the sampled search index of tsq_lookup.hip
//   K20a k_dc_offsets_ok     : an INDEX store's / a push's offsets start inside the bytes, never decrease and end inside them
//   K20b k_dc_keys_ascending : an INDEX store's keys strictly ascend under bytes.Compare
// tsq_dupcheck_push:
//   K20c k_dc_rebase         : the pushed offsets moved behind the bytes the handle already holds
// tsq_dupcheck_match, per stream:
//        tsq_groupid over the stream's keys (one TSQ_I64 or TSQ_BYTES column): exact ids, equality on the cells
//   K20d k_dc_words          : id << 32 | row of every row that takes part; tsq_sort's radix passes order them
//   K20e k_dc_prev           : the left neighbour in that order, when it has the same id, is prev_s
//   K20f k_dc_search_handle  : tsq_lk_find per row (tsq_lookup_dp.h: the descent tsq_lookup_task uses, in its per-row form)
//   K20g k_dc_search_index   : one lane per probe key, lower bound over the store's offsets with an 8-byte-piece compare, then equality
//   K20h k_dc_ord            : (REPLACE) the table row ordinal of an INDEX entry's handle
// then
//   K20i k_dc_first_error    : (INSERT) min over rows of row << 8 | first failing stream; one atomicMin per wave that has one
//   K20j k_dc_group_first    : (INSERT, after an in-batch conflict) the first row of the failing key's group
//   K20k k_dc_cand           : (REPLACE) the row EqualDatums must be asked about: statement row max_s prev_s, else the first stream's stored row
// tsq_dupcheck_resolve:
//   K20l k_dc_added          : added = !(candidate && equal); per stream the group's last added row (atomicMax, one per wave where its lanes
//                              agree on the group); the ordinals added rows match
//   K20m k_dc_put            : removed again = added and a later added row in one of its groups; put; the counts by wave reduction
//        tsq_launch_scan64   : added -> the position among the added rows
//   K20n k_dc_handles        : rowid_base + position + 1
//        tsq_sort + K20o k_dc_uniq_flag + tsq_launch_scan64 + K20p k_dc_uniq_scatter: the distinct matched ordinals, ascending
// tsq_rows_equal:
//   K20q k_rows_equal        : a lane per row pair, column after column, early exit
// No kernel waits on another workgroup; every result is written with plain vector stores.
#include "tsq_stage.h"
#include "tsq_lookup_dp.h"
#include "tsq_dupcheck_dp.h"

#include <memory>

#define DC_NONE INT64_MAX
#define DC_NO_GID 0xffffffffu

#define DC_ROWS(r, n) for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < (n); r += (int64_t)gridDim.x * blockDim.x)

// bit 0: an offset outside [0, n_bytes]; bit 1: an offset pair that decreases
__global__ void __launch_bounds__(256) k_dc_offsets_ok(const int64_t* offs, int64_t n, int64_t n_bytes, unsigned int* bad) {
    unsigned int e = 0;
    DC_ROWS(i, n + 1) {
        const int64_t o = offs[i];
        if (o < 0 || o > n_bytes) e |= 1u;
        if (i < n && offs[i + 1] < o) e |= 2u;
    }
    if (e) atomicOr(bad, e);
}
__global__ void __launch_bounds__(256) k_dc_keys_ascending(const uint8_t* keys, const int64_t* offs, int64_t n, unsigned int* bad) {
    bool b = false;
    DC_ROWS(i, n - 1) {
        const int64_t o0 = offs[i], o1 = offs[i + 1], o2 = offs[i + 2];
        b = b || !(tsq_dc_key_cmp(keys + o0, o1 - o0, keys + o1, o2 - o1) < 0);
    }
    if (b) atomicOr(bad, 4u);
}
__global__ void __launch_bounds__(256) k_dc_rebase(int64_t* dst, const int64_t* src, int64_t n_entries, int64_t delta) {
    DC_ROWS(i, n_entries) dst[i] = src[i] + delta;
}

__global__ void __launch_bounds__(256) k_dc_words(const uint64_t* gid64, const uint8_t* part, int64_t n, uint32_t* gid, int64_t* words) {
    DC_ROWS(r, n) {
        const bool p = !part || part[r];
        const uint32_t g = (uint32_t)gid64[r];
        gid[r] = p ? g : DC_NO_GID;
        words[r] = p ? (int64_t)(((uint64_t)g << 32) | (uint64_t)r) : DC_NONE;
    }
}
__global__ void __launch_bounds__(256) k_dc_prev(const int64_t* sorted, int64_t n, int32_t* prev) {
    DC_ROWS(i, n) {
        const int64_t w = sorted[i];
        if (w == DC_NONE) continue;
        const int64_t r = (int64_t)(uint32_t)w;
        if (r >= n) continue;
        const int64_t l = i > 0 ? sorted[i - 1] : DC_NONE;
        prev[r] = (l != DC_NONE && (l >> 32) == (w >> 32)) ? (int32_t)(uint32_t)l : -1;
    }
}
__global__ void __launch_bounds__(256) k_dc_search_handle(tsq_lk_index ix, const int64_t* keys, int64_t n, int64_t* ent) {
    DC_ROWS(r, n) ent[r] = tsq_lk_find(ix, ix.lv[ix.levels], keys[r]);
}
__global__ void __launch_bounds__(256) k_dc_search_index(const uint8_t* skeys, const int64_t* soffs, int64_t sn, const uint8_t* pkeys, const int64_t* poffs,
                                                         const uint8_t* part, int64_t n, int64_t* ent) {
    DC_ROWS(r, n) {
        int64_t e = -1;
        if (part[r] && sn > 0) {
            const int64_t b = poffs[r];
            e = tsq_dc_key_find(skeys, soffs, sn, pkeys + b, poffs[r + 1] - b);
        }
        ent[r] = e;
    }
}
// bit 3: an index entry whose handle is not a row of the table
__global__ void __launch_bounds__(256) k_dc_ord(tsq_lk_index ix, const int64_t* ent, const int64_t* entry_handles, int64_t n_entries, int64_t n, int64_t* ord,
                                                unsigned int* bad) {
    bool b = false;
    DC_ROWS(r, n) {
        const int64_t e = ent[r];
        int64_t o = -1;
        if (e >= 0 && e < n_entries) {
            o = tsq_lk_find(ix, ix.lv[ix.levels], entry_handles[e]);
            b = b || o < 0;
        }
        ord[r] = o;
    }
    if (b) atomicOr(bad, 8u);
}

struct DcStreams {
    int32_t n_streams;
    int32_t _pad;
    const int32_t* prev[TSQ_DUP_MAX_STREAMS];
    const int64_t* ent[TSQ_DUP_MAX_STREAMS];
    const int64_t* ord[TSQ_DUP_MAX_STREAMS];
    const uint32_t* gid[TSQ_DUP_MAX_STREAMS];
    int32_t* gmax[TSQ_DUP_MAX_STREAMS];
    const int64_t* entry_handles[TSQ_DUP_MAX_STREAMS];  // handle of entry e of the stream's store
    int64_t n_entries[TSQ_DUP_MAX_STREAMS];
};

__global__ void __launch_bounds__(256) k_dc_first_error(DcStreams s, int64_t n, unsigned long long* word) {
    unsigned long long best = ~0ull;
    DC_ROWS(r, n) {
        for (int k = 0; k < s.n_streams; k++)
            if (s.ent[k][r] >= 0 || s.prev[k][r] >= 0) {
                const unsigned long long w = ((unsigned long long)r << 8) | (unsigned long long)k;
                best = w < best ? w : best;
                break;
            }
    }
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(best, o, 64);
        best = y < best ? y : best;
    }
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(word, best);
}
__global__ void __launch_bounds__(256) k_dc_group_first(const uint32_t* gid, int64_t n, uint32_t target, unsigned long long* word) {
    unsigned long long best = ~0ull;
    DC_ROWS(r, n)
        if (gid[r] == target) best = (unsigned long long)r < best ? (unsigned long long)r : best;
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long y = __shfl_xor(best, o, 64);
        best = y < best ? y : best;
    }
    if ((threadIdx.x & 63) == 0 && best != ~0ull) atomicMin(word, best);
}
// kind: 0 none, 1 statement row, 2 stored row; counts[0] = rows of kind 1, counts[1] = rows of kind 2
__global__ void __launch_bounds__(256) k_dc_cand(DcStreams s, int64_t n, int64_t* cand_row, int64_t* cand_handle, int64_t* cand_ord, uint8_t* kind,
                                                 unsigned long long* counts) {
    unsigned int c1 = 0, c2 = 0;
    DC_ROWS(r, n) {
        int32_t j = -1;
        for (int k = 0; k < s.n_streams; k++) {
            const int32_t p = s.prev[k][r];
            j = p > j ? p : j;
        }
        int64_t h = 0, o = -1;
        uint8_t kd = 0;
        if (j >= 0) {
            kd = 1;
        } else {
            for (int k = 0; k < s.n_streams; k++) {
                const int64_t e = s.ent[k][r];
                if (e >= 0 && e < s.n_entries[k]) {
                    kd = 2;
                    h = s.entry_handles[k][e];
                    o = s.ord[k][r];
                    break;
                }
            }
        }
        cand_row[r] = j;
        cand_handle[r] = h;
        cand_ord[r] = o;
        kind[r] = kd;
        c1 += kd == 1;
        c2 += kd == 2;
    }
    for (int o = 32; o > 0; o >>= 1) {
        c1 += __shfl_xor(c1, o, 64);
        c2 += __shfl_xor(c2, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (c1) atomicAdd(counts, (unsigned long long)c1);
        if (c2) atomicAdd(counts + 1, (unsigned long long)c2);
    }
}

// The group's last added row: where the lanes of a wave that want an atomicMax agree on the group (runs of equal keys: "all rows identical"
// sends every row of a stream to one address), the highest such lane holds the largest row and issues the only one; otherwise one per row.
// The row loop is wave uniform (r0 is the wave's first row of the step), so the ballot and the shuffle see every lane.
__global__ void __launch_bounds__(256) k_dc_added(DcStreams s, int64_t n, const uint8_t* kind, const uint8_t* equal, uint8_t* added, uint8_t* added_out,
                                                  int64_t* rem_words) {
    const int lane = threadIdx.x & 63;
    for (int64_t r0 = (int64_t)blockIdx.x * blockDim.x + threadIdx.x - lane; r0 < n; r0 += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = r0 + lane;
        const bool in = r < n;
        bool a = false;
        if (in) {
            a = !(kind[r] && equal[r]);
            added[r] = a;
            added_out[r] = a;
        }
        for (int k = 0; k < s.n_streams; k++) {
            uint32_t g = DC_NO_GID;
            if (in) {
                const int64_t o = s.ord[k][r];
                rem_words[r * s.n_streams + k] = (a && o >= 0) ? o : DC_NONE;
                g = s.gid[k][r];
            }
            const bool want = in && a && g != DC_NO_GID && (int64_t)g < n;
            const unsigned long long m = __ballot(want);
            if (m) {  // (wave uniform)
                const int top = 63 - __clzll((long long)m);
                const uint32_t gt = (uint32_t)__shfl((int)g, top, 64);
                const bool same = __all(!want || g == gt);
                if (same ? lane == top : want) atomicMax(&s.gmax[k][g], (int32_t)r);
            }
        }
    }
}
// counts[2] = added rows, counts[3] = added rows that a later added row removes again
__global__ void __launch_bounds__(256) k_dc_put(DcStreams s, int64_t n, const uint8_t* added, uint8_t* put, int64_t* scanv, unsigned long long* counts) {
    unsigned int ca = 0, cr = 0;
    DC_ROWS(r, n) {
        const bool a = added[r];
        bool rem = false;
        for (int k = 0; k < s.n_streams; k++) {
            const uint32_t g = s.gid[k][r];
            if (a && g != DC_NO_GID && (int64_t)g < n) rem = rem || (int64_t)s.gmax[k][g] > r;
        }
        put[r] = a && !rem;
        scanv[r] = a ? 1 : 0;
        ca += a;
        cr += a && rem;
    }
    for (int o = 32; o > 0; o >>= 1) {
        ca += __shfl_xor(ca, o, 64);
        cr += __shfl_xor(cr, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (ca) atomicAdd(counts + 2, (unsigned long long)ca);
        if (cr) atomicAdd(counts + 3, (unsigned long long)cr);
    }
}
__global__ void __launch_bounds__(256) k_dc_handles(const uint8_t* added, const int64_t* pos, int64_t n, int64_t rowid_base, int64_t* handles_out) {
    DC_ROWS(r, n) handles_out[r] = added[r] ? (int64_t)((uint64_t)rowid_base + (uint64_t)pos[r] + 1u) : 0;
}
__global__ void __launch_bounds__(256) k_dc_uniq_flag(const int64_t* sorted, int64_t m, int64_t* flag) {
    DC_ROWS(i, m) {
        const int64_t w = sorted[i];
        flag[i] = (w != DC_NONE && (i == 0 || sorted[i - 1] != w)) ? 1 : 0;
    }
}
__global__ void __launch_bounds__(256) k_dc_uniq_scatter(const int64_t* sorted, const int64_t* pos, int64_t m, const int64_t* table_handles, int64_t n_table,
                                                         int64_t cap, int64_t* out_handles, int64_t* out_ords) {
    DC_ROWS(i, m) {
        const int64_t w = sorted[i];
        if (w == DC_NONE || (i > 0 && sorted[i - 1] == w)) continue;
        const int64_t at = pos[i];
        if (at < 0 || at >= cap) continue;
        out_ords[at] = w;
        out_handles[at] = (w >= 0 && w < n_table) ? table_handles[w] : 0;
    }
}

struct RowsEqualArgs {
    tsq_dc_col a[TSQ_MAX_COLS], b[TSQ_MAX_COLS];
    int32_t type[TSQ_MAX_COLS];
    int32_t n_cols;
    int32_t _pad;
    const int64_t* idx_a;  // nullptr: pair i takes row i
    const int64_t* idx_b;
    int64_t rows_a, rows_b, n;
    uint8_t* flags;
};
__global__ void __launch_bounds__(256) k_rows_equal(RowsEqualArgs q) {
    DC_ROWS(i, q.n) {
        const int64_t ra = q.idx_a ? q.idx_a[i] : i, rb = q.idx_b ? q.idx_b[i] : i;
        bool eq = ra >= 0 && rb >= 0 && ra < q.rows_a && rb < q.rows_b;
        for (int c = 0; eq && c < q.n_cols; c++) eq = tsq_dc_cell_equal(q.type[c], q.a[c], ra, q.b[c], rb);
        q.flags[i] = eq ? 1 : 0;
    }
}

// ====================================================================== host side
#define TSQ_MAGIC_DUPCHECK 0x74737144u /* 'tsqD' */

struct DcStream {
    int32_t kind = TSQ_DUP_HANDLE;
    // the store (the library's copies)
    int64_t sn = 0, sbytes = 0;
    DevBuf skeys, soffs, shandles;  // INDEX
    // the statement's keys
    DevBuf pkeys, poffs, pdist;  // INDEX: bytes, offsets[rows + 1], distinct flags
    DevBuf phandles;             // HANDLE
    int64_t pbytes = 0;
    // match results
    DevBuf gid, prev, ent, ord;
    DevBuf gmax;
};
struct tsq_dupcheck {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    std::atomic<int> cancelled{0};
    int32_t mode = TSQ_DUP_INSERT, n_streams = 0;
    DcStream st[TSQ_DUP_MAX_STREAMS];
    tsq_lookup* table = nullptr;  // the table's handles + their search index (tsq_lookup.hip)
    int64_t n_table = 0;
    int64_t rows = 0, pushes = 0;
    int state = 0;  // 0 taking pushes, 1 matched, 2 resolved
    DevBuf counters;  // 16 words
    DevBuf gid64, words, sorted, sorted_bm, scan_tmp, kind, added, scanv, rem_words;
    int64_t n_cand_batch = 0, n_cand_store = 0;
    double kernel_ms = 0;
    DevEvent ev[2];
    ~tsq_dupcheck() {  // the nested handle first; the buffers and events are released by their own destructors
        if (table) tsq_lookup_destroy(table);
    }
};

namespace {
tsq_status dc_cancelled(tsq_dupcheck* d) {
    if (d->cancelled.load()) return tsq_fail(&d->hdr, TSQ_ERR_CANCELLED, "dupcheck cancelled");
    return TSQ_OK;
}
// n signed 64-bit words (device) sorted ascending into d->sorted, by the radix passes of tsq_sort.hip
tsq_status dc_sort(tsq_dupcheck* d, const int64_t* src, int64_t n) {
    tsq_ctx* ctx = d->ctx;
    tsq_handle_hdr* h = &d->hdr;
    TSQ_TRY(d->sorted.reserve(ctx, h, (size_t)n * 8 + 64));
    TSQ_TRY(d->sorted_bm.reserve(ctx, h, tsq_bitmap_bytes(n) + 64));
    tsq_sort_cfg cfg;
    memset(&cfg, 0, sizeof cfg);
    cfg.n_cols = 1;
    cfg.col_types[0] = TSQ_I64;
    cfg.n_keys = 1;
    cfg.limit_count = -1;
    cfg.max_chunk_size = 1024;
    tsq_sort* s = nullptr;
    tsq_status st = tsq_sort_create(ctx, &cfg, &s);
    if (st != TSQ_OK) return tsq_fail(h, st, std::string("dupcheck: sort: ") + tsq_last_error(ctx));
    tsq_col in, out;
    memset(&in, 0, sizeof in);
    in.data = (void*)src;
    in.length = n;
    in.elem_size = 8;
    in.type = TSQ_I64;
    in.flags = TSQ_COL_DEVICE;
    out = in;
    out.data = d->sorted.p;
    out.null_bitmap = d->sorted_bm.as<uint8_t>();
    int64_t got = 0;
    int32_t eos = 0;
    st = tsq_sort_push(s, &in, 1, n);
    if (st == TSQ_OK) st = tsq_sort_finish(s);
    if (st == TSQ_OK) st = tsq_sort_pull(s, &out, 1, n, &got, &eos);
    if (st != TSQ_OK) tsq_fail(h, st, std::string("dupcheck: sort: ") + tsq_last_error(s));
    else if (got != n) st = tsq_fail(h, TSQ_ERR_HIP, "internal: the sort of the key words lost rows");
    tsq_sort_destroy(s);
    return st;
}
// exact group ids of one key column into d->gid64
tsq_status dc_group(tsq_dupcheck* d, const tsq_col* key, int64_t n) {
    tsq_ctx* ctx = d->ctx;
    tsq_handle_hdr* h = &d->hdr;
    TSQ_TRY(d->gid64.reserve(ctx, h, (size_t)n * 8 + 64));
    tsq_groupid* g = nullptr;
    const int32_t kt = key->type;
    tsq_status st = tsq_groupid_create(ctx, &kt, 1, n, &g);  // (at most n groups: the table is sized once, no growth pass)
    if (st != TSQ_OK) return tsq_fail(h, st, std::string("dupcheck: group ids: ") + tsq_last_error(ctx));
    st = tsq_groupid_assign(g, key, 1, n, d->gid64.as<uint64_t>());
    if (st != TSQ_OK) tsq_fail(h, st, std::string("dupcheck: group ids: ") + tsq_last_error(g));
    tsq_groupid_destroy(g);
    return st;
}
// reads `words` 64-bit words of the handle's counters into ctx->pinned + 48..
tsq_status dc_read_counters(tsq_dupcheck* d, int words) {
    tsq_ctx* ctx = d->ctx;
    TSQ_HIP(&d->hdr, hipMemcpyAsync(ctx->pinned + 48, d->counters.p, (size_t)words * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(&d->hdr, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}
void dc_fill_streams(tsq_dupcheck* d, DcStreams* s) {
    memset(s, 0, sizeof *s);
    s->n_streams = d->n_streams;
    const tsq_lk_index* ix = d->table ? tsq_lookup_index_of(d->table) : nullptr;
    for (int k = 0; k < d->n_streams; k++) {
        DcStream& t = d->st[k];
        s->prev[k] = t.prev.as<int32_t>();
        s->ent[k] = t.ent.as<int64_t>();
        s->ord[k] = t.kind == TSQ_DUP_HANDLE ? t.ent.as<int64_t>() : t.ord.as<int64_t>();
        s->gid[k] = t.gid.as<uint32_t>();
        s->gmax[k] = t.gmax.as<int32_t>();
        if (t.kind == TSQ_DUP_HANDLE) {
            s->entry_handles[k] = ix ? ix->lv[0] : nullptr;
            s->n_entries[k] = ix ? ix->n[0] : 0;
        } else {
            s->entry_handles[k] = t.shandles.as<int64_t>();
            s->n_entries[k] = t.sn;
        }
    }
}
}  // namespace

TSQ_API tsq_status tsq_dupcheck_create(tsq_ctx* ctx, const tsq_dup_stream* streams, int32_t n_streams, int32_t mode, const int64_t* table_handles,
                                       int64_t n_table_rows, tsq_dupcheck** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !out) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_dupcheck_create: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (!streams || n_streams < 1) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: no stream");
    if (n_streams > TSQ_DUP_MAX_STREAMS) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: more than TSQ_DUP_MAX_STREAMS streams");
    if (mode != TSQ_DUP_INSERT && mode != TSQ_DUP_REPLACE) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: bad mode");
    int handle_stream = -1;
    for (int k = 0; k < n_streams; k++) {
        const tsq_dup_stream& s = streams[k];
        if (s.kind != TSQ_DUP_HANDLE && s.kind != TSQ_DUP_INDEX) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: bad stream kind");
        if (s.n < 0 || (s.n > 0 && !s.handles)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: bad handle array");
        if (s.kind == TSQ_DUP_HANDLE) {
            if (handle_stream >= 0) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: two HANDLE streams");
            handle_stream = k;
        } else {
            if (s.key_bytes < 0 || (s.n > 0 && !s.key_offsets) || (s.key_bytes > 0 && !s.keys))
                return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: bad index keys");
            if (mode == TSQ_DUP_REPLACE && (s.flags & TSQ_DUP_FLOAT_KEY))
                return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "REPLACE over a unique index with a FLOAT / DOUBLE column: equal rows may have different keys");
        }
    }
    if (handle_stream >= 0) {
        table_handles = streams[handle_stream].handles;
        n_table_rows = streams[handle_stream].n;
    }
    if (n_table_rows < 0 || (n_table_rows > 0 && !table_handles)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_dupcheck_create: bad table handles");
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    std::unique_ptr<tsq_dupcheck> d(new tsq_dupcheck());
    d->hdr.magic = TSQ_MAGIC_DUPCHECK;
    d->ctx = ctx;
    d->mode = mode;
    d->n_streams = n_streams;
    d->n_table = n_table_rows;
    tsq_status st = TSQ_OK;
    std::string msg;
    auto fail = [&](tsq_status s, const std::string& m) {
        st = s;
        msg = m;
    };
    for (int i = 0; i < 2 && st == TSQ_OK; i++)
        if (d->ev[i].create() != hipSuccess) fail(TSQ_ERR_HIP, "hipEventCreate");
    if (st == TSQ_OK && (st = d->counters.reserve(ctx, ch, 16 * 8)) != TSQ_OK) msg = ch->err;
    if (st == TSQ_OK) {
        st = tsq_lookup_create(ctx, table_handles, n_table_rows, TSQ_COL_DEVICE, &d->table);  // copy, "table handles not ascending", search index
        if (st != TSQ_OK) msg = tsq_last_error(ctx);
    }
    unsigned int* bad = d->counters.as<unsigned int>();
    for (int k = 0; k < n_streams && st == TSQ_OK; k++) {
        const tsq_dup_stream& s = streams[k];
        DcStream& t = d->st[k];
        t.kind = s.kind;
        if (s.kind == TSQ_DUP_HANDLE) continue;
        t.sn = s.n;
        t.sbytes = s.key_bytes;
        if ((st = t.skeys.reserve(ctx, ch, (size_t)s.key_bytes + 64)) != TSQ_OK || (st = t.soffs.reserve(ctx, ch, ((size_t)s.n + 1) * 8 + 64)) != TSQ_OK ||
            (st = t.shandles.reserve(ctx, ch, (size_t)s.n * 8 + 64)) != TSQ_OK) {
            msg = ch->err;
            break;
        }
        hipError_t e = hipMemsetAsync(t.soffs.p, 0, 8, ctx->stream);
        if (e == hipSuccess && s.n > 0) e = hipMemcpyAsync(t.soffs.p, s.key_offsets, ((size_t)s.n + 1) * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess && s.n > 0) e = hipMemcpyAsync(t.shandles.p, s.handles, (size_t)s.n * 8, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess && s.key_bytes > 0) e = hipMemcpyAsync(t.skeys.p, s.keys, (size_t)s.key_bytes, hipMemcpyDeviceToDevice, ctx->stream);
        if (e == hipSuccess) e = hipMemsetAsync(bad, 0, 8, ctx->stream);
        if (e == hipSuccess && s.n > 0) {
            hipLaunchKernelGGL(k_dc_offsets_ok, dim3(tsq_grid_for(ctx, s.n + 1, 256)), dim3(256), 0, ctx->stream, t.soffs.as<int64_t>(), s.n, s.key_bytes, bad);
            e = hipGetLastError();
        }
        if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned + 48, bad, 8, hipMemcpyDeviceToHost, ctx->stream);
        if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
        if (e == hipSuccess && (ctx->pinned[48] & 3u)) {
            fail(TSQ_ERR_INVALID, "tsq_dupcheck_create: index key offsets decrease or leave the keys");
            break;
        }
        if (e == hipSuccess && s.n > 1) {  // (only now: the offsets are known to stay inside the keys)
            hipLaunchKernelGGL(k_dc_keys_ascending, dim3(tsq_grid_for(ctx, s.n - 1, 256)), dim3(256), 0, ctx->stream, t.skeys.as<uint8_t>(), t.soffs.as<int64_t>(),
                               s.n, bad);
            e = hipGetLastError();
            if (e == hipSuccess) e = hipMemcpyAsync(ctx->pinned + 48, bad, 8, hipMemcpyDeviceToHost, ctx->stream);
            if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
            if (e == hipSuccess && (ctx->pinned[48] & 4u)) {
                fail(TSQ_ERR_INVALID, "index keys not ascending");
                break;
            }
        }
        if (e != hipSuccess) fail(TSQ_ERR_HIP, std::string("tsq_dupcheck_create: ") + hipGetErrorString(e));
    }
    if (st != TSQ_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return tsq_fail(ch, st, msg);
    }
    *out = d.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_dupcheck_push(tsq_dupcheck* d, const tsq_dup_keys* keys, int32_t n_streams, int64_t n) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(d, TSQ_MAGIC_DUPCHECK));
    if (!d || d->hdr.magic != TSQ_MAGIC_DUPCHECK) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &d->hdr;
    TSQ_TRY(dc_cancelled(d));
    if (d->state != 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_push: after tsq_dupcheck_match");
    if (n < 0 || n_streams != d->n_streams || (n > 0 && !keys)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_push: bad arguments");
    if (d->rows + n >= (1LL << 31) || (d->rows + n) * d->n_streams >= (1LL << 31))
        return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "dupcheck: 2^31 statement rows (times streams) or more");
    d->pushes++;
    if (n == 0) return TSQ_OK;
    tsq_ctx* ctx = d->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    for (int k = 0; k < d->n_streams; k++) {
        const tsq_dup_keys& p = keys[k];
        if (d->st[k].kind == TSQ_DUP_HANDLE ? !p.handles : (!p.key_offsets || p.key_bytes < 0 || (p.key_bytes > 0 && !p.keys)))
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_push: a stream's keys are missing");
    }
    // the offsets of every INDEX stream are checked before anything is appended: a refused push leaves the handle as it was
    unsigned int* bad = d->counters.as<unsigned int>();
    int64_t first[TSQ_DUP_MAX_STREAMS], last[TSQ_DUP_MAX_STREAMS];
    for (int k = 0; k < d->n_streams; k++) {
        first[k] = last[k] = 0;
        if (d->st[k].kind != TSQ_DUP_INDEX) continue;
        const tsq_dup_keys& p = keys[k];
        TSQ_HIP(h, hipMemsetAsync(bad, 0, 8, ctx->stream));
        hipLaunchKernelGGL(k_dc_offsets_ok, dim3(tsq_grid_for(ctx, n + 1, 256)), dim3(256), 0, ctx->stream, p.key_offsets, n, p.key_bytes, bad);
        TSQ_HIP(h, hipGetLastError());
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 48, bad, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 49, p.key_offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 50, p.key_offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        if (ctx->pinned[48] & 3u) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_push: key offsets decrease or leave the keys");
        first[k] = (int64_t)ctx->pinned[49];
        last[k] = (int64_t)ctx->pinned[50];
    }
    const int64_t r0 = d->rows;
    for (int k = 0; k < d->n_streams; k++) {
        DcStream& t = d->st[k];
        const tsq_dup_keys& p = keys[k];
        if (t.kind == TSQ_DUP_HANDLE) {
            TSQ_TRY(t.phandles.reserve(ctx, h, (size_t)(r0 + n) * 8 + 64, true, (size_t)r0 * 8));
            TSQ_HIP(h, hipMemcpyAsync(t.phandles.as<int64_t>() + r0, p.handles, (size_t)n * 8, hipMemcpyDeviceToDevice, ctx->stream));
            continue;
        }
        const int64_t nb = last[k] - first[k];
        TSQ_TRY(t.pkeys.reserve(ctx, h, (size_t)(t.pbytes + nb) + 64, true, (size_t)t.pbytes));
        TSQ_TRY(t.poffs.reserve(ctx, h, (size_t)(r0 + n + 1) * 8 + 64, true, (size_t)(r0 + 1) * 8));
        TSQ_TRY(t.pdist.reserve(ctx, h, (size_t)(r0 + n) + 64, true, (size_t)r0));
        if (nb > 0) TSQ_HIP(h, hipMemcpyAsync(t.pkeys.as<uint8_t>() + t.pbytes, p.keys + first[k], (size_t)nb, hipMemcpyDeviceToDevice, ctx->stream));
        hipLaunchKernelGGL(k_dc_rebase, dim3(tsq_grid_for(ctx, n + 1, 256)), dim3(256), 0, ctx->stream, t.poffs.as<int64_t>() + r0, p.key_offsets, n + 1,
                           t.pbytes - first[k]);
        TSQ_HIP(h, hipGetLastError());
        if (p.distinct) TSQ_HIP(h, hipMemcpyAsync(t.pdist.as<uint8_t>() + r0, p.distinct, (size_t)n, hipMemcpyDeviceToDevice, ctx->stream));
        else TSQ_HIP(h, hipMemsetAsync(t.pdist.as<uint8_t>() + r0, 1, (size_t)n, ctx->stream));
        t.pbytes += nb;
    }
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // the caller may reuse its buffers
    d->rows += n;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_dupcheck_match(tsq_dupcheck* d, tsq_dup_conflict* conflict, int64_t* cand_row, int64_t* cand_handle, int64_t* cand_ord,
                                      int64_t* n_cand_batch, int64_t* n_cand_store) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(d, TSQ_MAGIC_DUPCHECK));
    if (!d || d->hdr.magic != TSQ_MAGIC_DUPCHECK) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &d->hdr;
    if (n_cand_batch) *n_cand_batch = 0;
    if (n_cand_store) *n_cand_store = 0;
    if (conflict) memset(conflict, 0, sizeof *conflict);
    TSQ_TRY(dc_cancelled(d));
    if (d->state != 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_match: called twice");
    const int64_t n = d->rows;
    const bool replace = d->mode == TSQ_DUP_REPLACE;
    if (replace ? (n > 0 && (!cand_row || !cand_handle || !cand_ord)) : !conflict) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_match: bad arguments");
    if (n == 0) {
        d->state = 1;
        return TSQ_OK;
    }
    tsq_ctx* ctx = d->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    TSQ_HIP(h, hipEventRecord(d->ev[0], ctx->stream));
    const tsq_lk_index ix = *tsq_lookup_index_of(d->table);
    const int grid = tsq_grid_for(ctx, n, 256);
    unsigned long long* cnt = d->counters.as<unsigned long long>();
    TSQ_HIP(h, hipMemsetAsync(cnt, 0, 16 * 8, ctx->stream));
    TSQ_TRY(d->words.reserve(ctx, h, (size_t)n * 8 + 64));
    for (int k = 0; k < d->n_streams; k++) {
        DcStream& t = d->st[k];
        TSQ_TRY(t.gid.reserve(ctx, h, (size_t)n * 4 + 64));
        TSQ_TRY(t.prev.reserve(ctx, h, (size_t)n * 4 + 64));
        TSQ_TRY(t.ent.reserve(ctx, h, (size_t)n * 8 + 64));
        tsq_col key;
        memset(&key, 0, sizeof key);
        key.length = n;
        key.flags = TSQ_COL_DEVICE;
        if (t.kind == TSQ_DUP_HANDLE) {
            key.data = t.phandles.p;
            key.elem_size = 8;
            key.type = TSQ_I64;
        } else {
            key.data = t.pkeys.p;
            key.offsets = t.poffs.as<int64_t>();
            key.elem_size = -1;
            key.type = TSQ_BYTES;
        }
        TSQ_TRY(dc_group(d, &key, n));
        const uint8_t* part = t.kind == TSQ_DUP_INDEX ? t.pdist.as<uint8_t>() : nullptr;
        hipLaunchKernelGGL(k_dc_words, dim3(grid), dim3(256), 0, ctx->stream, d->gid64.as<uint64_t>(), part, n, t.gid.as<uint32_t>(), d->words.as<int64_t>());
        TSQ_HIP(h, hipGetLastError());
        TSQ_TRY(dc_sort(d, d->words.as<int64_t>(), n));
        TSQ_HIP(h, hipMemsetAsync(t.prev.p, 0xff, (size_t)n * 4, ctx->stream));
        hipLaunchKernelGGL(k_dc_prev, dim3(grid), dim3(256), 0, ctx->stream, d->sorted.as<int64_t>(), n, t.prev.as<int32_t>());
        if (t.kind == TSQ_DUP_HANDLE) {
            hipLaunchKernelGGL(k_dc_search_handle, dim3(grid), dim3(256), 0, ctx->stream, ix, t.phandles.as<int64_t>(), n, t.ent.as<int64_t>());
        } else {
            hipLaunchKernelGGL(k_dc_search_index, dim3(grid), dim3(256), 0, ctx->stream, t.skeys.as<uint8_t>(), t.soffs.as<int64_t>(), t.sn, t.pkeys.as<uint8_t>(),
                               t.poffs.as<int64_t>(), t.pdist.as<uint8_t>(), n, t.ent.as<int64_t>());
            if (replace) {
                TSQ_TRY(t.ord.reserve(ctx, h, (size_t)n * 8 + 64));
                hipLaunchKernelGGL(k_dc_ord, dim3(grid), dim3(256), 0, ctx->stream, ix, t.ent.as<int64_t>(), t.shandles.as<int64_t>(), t.sn, n, t.ord.as<int64_t>(),
                                   (unsigned int*)(cnt + 4));
            }
        }
        TSQ_HIP(h, hipGetLastError());
    }
    DcStreams s;
    dc_fill_streams(d, &s);
    if (!replace) {
        TSQ_HIP(h, hipMemsetAsync(cnt, 0xff, 16, ctx->stream));
        hipLaunchKernelGGL(k_dc_first_error, dim3(grid), dim3(256), 0, ctx->stream, s, n, cnt);
        TSQ_HIP(h, hipGetLastError());
        TSQ_HIP(h, hipEventRecord(d->ev[1], ctx->stream));
        TSQ_TRY(dc_read_counters(d, 1));
        float ms = 0;
        if (hipEventElapsedTime(&ms, d->ev[0], d->ev[1]) == hipSuccess) d->kernel_ms += ms;
        d->state = 1;
        const uint64_t w = ctx->pinned[48];
        if (w == ~0ull) return TSQ_OK;
        const int64_t row = (int64_t)(w >> 8);
        const int k = (int)(w & 0xff);
        if (row >= n || k >= d->n_streams) return tsq_fail(h, TSQ_ERR_HIP, "internal: first-error word out of range");
        DcStream& t = d->st[k];
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 49, t.ent.as<int64_t>() + row, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 50, t.gid.as<uint32_t>() + row, 4, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        const int64_t e = (int64_t)ctx->pinned[49];
        conflict->row = row;
        conflict->stream = k;
        conflict->dup_row = -1;
        if (e >= 0) {  // a stored entry was there first
            if (e >= s.n_entries[k]) return tsq_fail(h, TSQ_ERR_HIP, "internal: matched entry out of range");
            conflict->from_store = 1;
            TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 51, s.entry_handles[k] + e, 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
            conflict->dup_handle = (int64_t)ctx->pinned[51];
        } else {  // the FIRST row of the key's group wrote the entry
            const uint32_t target = (uint32_t)ctx->pinned[50];
            hipLaunchKernelGGL(k_dc_group_first, dim3(grid), dim3(256), 0, ctx->stream, t.gid.as<uint32_t>(), n, target, cnt + 1);
            TSQ_HIP(h, hipGetLastError());
            TSQ_TRY(dc_read_counters(d, 2));
            conflict->dup_row = (int64_t)ctx->pinned[49];
            if (conflict->dup_row < 0 || conflict->dup_row >= row) return tsq_fail(h, TSQ_ERR_HIP, "internal: in-batch conflict without an earlier row");
        }
        return tsq_fail(h, TSQ_ERR_KEY_EXISTS, "duplicate entry: statement row " + std::to_string(row) + ", stream " + std::to_string(k));
    }
    TSQ_TRY(d->kind.reserve(ctx, h, (size_t)n + 64));
    hipLaunchKernelGGL(k_dc_cand, dim3(grid), dim3(256), 0, ctx->stream, s, n, cand_row, cand_handle, cand_ord, d->kind.as<uint8_t>(), cnt);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(d->ev[1], ctx->stream));
    TSQ_TRY(dc_read_counters(d, 5));
    float ms = 0;
    if (hipEventElapsedTime(&ms, d->ev[0], d->ev[1]) == hipSuccess) d->kernel_ms += ms;
    if (ctx->pinned[52] & 8u) return tsq_fail(h, TSQ_ERR_INVALID, "dupcheck: an index entry's handle is not a row of the table");
    d->n_cand_batch = (int64_t)ctx->pinned[48];
    d->n_cand_store = (int64_t)ctx->pinned[49];
    if (n_cand_batch) *n_cand_batch = d->n_cand_batch;
    if (n_cand_store) *n_cand_store = d->n_cand_store;
    d->state = 1;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_dupcheck_resolve(tsq_dupcheck* d, const uint8_t* equal_flags, int64_t rowid_base, uint8_t* added_out, uint8_t* put_out,
                                        int64_t* handles_out, int64_t* removed_handles, int64_t* removed_ords, int64_t cap_removed,
                                        tsq_dup_result* result) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(d, TSQ_MAGIC_DUPCHECK));
    if (!d || d->hdr.magic != TSQ_MAGIC_DUPCHECK) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &d->hdr;
    if (result) memset(result, 0, sizeof *result);
    TSQ_TRY(dc_cancelled(d));
    if (d->mode != TSQ_DUP_REPLACE) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_resolve: the handle is in INSERT mode");
    if (d->state < 1) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_resolve: before tsq_dupcheck_match");
    const int64_t n = d->rows;
    if (!result || cap_removed < 0 || (cap_removed > 0 && (!removed_handles || !removed_ords)) || (n > 0 && (!equal_flags || !added_out || !put_out)))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_resolve: bad arguments");
    result->rowid_base = rowid_base;
    if (n == 0) {
        d->state = 2;
        return TSQ_OK;
    }
    tsq_ctx* ctx = d->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    TSQ_HIP(h, hipEventRecord(d->ev[0], ctx->stream));
    const int S = d->n_streams;
    const int64_t m = n * S;
    const int grid = tsq_grid_for(ctx, n, 256);
    unsigned long long* cnt = d->counters.as<unsigned long long>();
    TSQ_HIP(h, hipMemsetAsync(cnt, 0, 16 * 8, ctx->stream));
    TSQ_TRY(d->added.reserve(ctx, h, (size_t)n + 64));
    TSQ_TRY(d->scanv.reserve(ctx, h, (size_t)(m + 1) * 8 + 64));
    TSQ_TRY(d->rem_words.reserve(ctx, h, (size_t)m * 8 + 64));
    for (int k = 0; k < S; k++) {
        TSQ_TRY(d->st[k].gmax.reserve(ctx, h, (size_t)n * 4 + 64));
        TSQ_HIP(h, hipMemsetAsync(d->st[k].gmax.p, 0xff, (size_t)n * 4, ctx->stream));
    }
    DcStreams s;
    dc_fill_streams(d, &s);
    hipLaunchKernelGGL(k_dc_added, dim3(grid), dim3(256), 0, ctx->stream, s, n, d->kind.as<uint8_t>(), equal_flags, d->added.as<uint8_t>(), added_out,
                       d->rem_words.as<int64_t>());
    hipLaunchKernelGGL(k_dc_put, dim3(grid), dim3(256), 0, ctx->stream, s, n, d->added.as<uint8_t>(), put_out, d->scanv.as<int64_t>(), cnt);
    TSQ_HIP(h, hipGetLastError());
    if (handles_out) {
        TSQ_TRY(tsq_launch_scan64(ctx, h, d->scanv.as<int64_t>(), n, d->scan_tmp));
        hipLaunchKernelGGL(k_dc_handles, dim3(grid), dim3(256), 0, ctx->stream, d->added.as<uint8_t>(), d->scanv.as<int64_t>(), n, rowid_base, handles_out);
        TSQ_HIP(h, hipGetLastError());
    }
    int64_t n_removed_store = 0;
    if (d->n_table > 0) {  // (an empty table has no row to remove)
        TSQ_TRY(dc_sort(d, d->rem_words.as<int64_t>(), m));
        const int gm = tsq_grid_for(ctx, m, 256);
        hipLaunchKernelGGL(k_dc_uniq_flag, dim3(gm), dim3(256), 0, ctx->stream, d->sorted.as<int64_t>(), m, d->scanv.as<int64_t>());
        TSQ_HIP(h, hipGetLastError());
        TSQ_TRY(tsq_launch_scan64(ctx, h, d->scanv.as<int64_t>(), m, d->scan_tmp));
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 56, d->scanv.as<int64_t>() + m, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        n_removed_store = (int64_t)ctx->pinned[56];
        result->n_removed_store = n_removed_store;
        if (n_removed_store > cap_removed) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_dupcheck_resolve: removed-row buffers too small (n_removed_store = rows needed)");
        if (n_removed_store > 0) {
            const tsq_lk_index* ix = tsq_lookup_index_of(d->table);
            hipLaunchKernelGGL(k_dc_uniq_scatter, dim3(gm), dim3(256), 0, ctx->stream, d->sorted.as<int64_t>(), d->scanv.as<int64_t>(), m, ix->lv[0], ix->n[0],
                               cap_removed, removed_handles, removed_ords);
            TSQ_HIP(h, hipGetLastError());
        }
    }
    TSQ_HIP(h, hipEventRecord(d->ev[1], ctx->stream));
    TSQ_TRY(dc_read_counters(d, 4));
    float ms = 0;
    if (hipEventElapsedTime(&ms, d->ev[0], d->ev[1]) == hipSuccess) d->kernel_ms += ms;
    result->n_added = (int64_t)ctx->pinned[50];
    result->n_removed_batch = (int64_t)ctx->pinned[51];
    result->n_put = result->n_added - result->n_removed_batch;
    result->affected = n + n_removed_store + result->n_removed_batch;
    result->rowid_base = (int64_t)((uint64_t)rowid_base + (uint64_t)result->n_added);
    d->state = 2;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_dupcheck_reset(tsq_dupcheck* d) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(d, TSQ_MAGIC_DUPCHECK));
    if (!d || d->hdr.magic != TSQ_MAGIC_DUPCHECK) return TSQ_ERR_INVALID;
    TSQ_TRY(dc_cancelled(d));
    (void)hipStreamSynchronize(d->ctx->stream);
    for (auto& t : d->st) t.pbytes = 0;
    d->rows = 0;
    d->state = 0;
    d->n_cand_batch = d->n_cand_store = 0;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_dupcheck_stats(tsq_dupcheck* d, int64_t* rows, int64_t* pushes, int64_t* cand_batch, int64_t* cand_store, double* kernel_ms) {
    if (!d || d->hdr.magic != TSQ_MAGIC_DUPCHECK) return TSQ_ERR_INVALID;
    if (rows) *rows = d->rows;
    if (pushes) *pushes = d->pushes;
    if (cand_batch) *cand_batch = d->n_cand_batch;
    if (cand_store) *cand_store = d->n_cand_store;
    if (kernel_ms) *kernel_ms = d->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_dupcheck_cancel(tsq_dupcheck* d) {
    if (!d || d->hdr.magic != TSQ_MAGIC_DUPCHECK) return TSQ_ERR_INVALID;
    d->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_dupcheck_destroy(tsq_dupcheck* d) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(d, TSQ_MAGIC_DUPCHECK));
    if (!d || d->hdr.magic != TSQ_MAGIC_DUPCHECK) return;
    (void)hipSetDevice(d->ctx->device);
    (void)hipStreamSynchronize(d->ctx->stream);
    d->hdr.magic = 0;
    delete d;
}

TSQ_API tsq_status tsq_rows_equal(tsq_ctx* ctx, const tsq_col* cols_a, const int64_t* idx_a, const tsq_col* cols_b, const int64_t* idx_b, int32_t n_cols,
                                  int64_t n, uint8_t* flags_out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &ctx->hdr;
    if (n < 0 || n_cols < 0 || (n_cols > 0 && (!cols_a || !cols_b)) || (n > 0 && !flags_out)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_equal: bad arguments");
    if (n_cols > TSQ_MAX_COLS) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_rows_equal: more than TSQ_MAX_COLS columns");
    if (n >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_rows_equal: 2^31 row pairs or more");
    RowsEqualArgs q;
    memset(&q, 0, sizeof q);
    q.n_cols = n_cols;
    q.rows_a = n_cols > 0 ? cols_a[0].length : (idx_a ? 0 : n);
    q.rows_b = n_cols > 0 ? cols_b[0].length : (idx_b ? 0 : n);
    for (int c = 0; c < n_cols; c++) {
        const tsq_col &a = cols_a[c], &b = cols_b[c];
        if (a.type != b.type || a.type < TSQ_I64 || a.type > TSQ_BYTES) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_equal: the two sides' column types differ");
        if (!(a.flags & TSQ_COL_DEVICE) || !(b.flags & TSQ_COL_DEVICE)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_equal: columns must be device resident (TSQ_COL_DEVICE)");
        if (a.length != q.rows_a || b.length != q.rows_b || a.length < 0 || b.length < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_equal: column lengths differ");
        if ((a.length > 0 && (!a.data && a.type != TSQ_BYTES)) || (b.length > 0 && (!b.data && b.type != TSQ_BYTES)) ||
            (a.type == TSQ_BYTES && ((a.length > 0 && !a.offsets) || (b.length > 0 && !b.offsets))))
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_rows_equal: a column without data / offsets");
        q.type[c] = a.type;
        q.a[c] = {a.data, a.null_bitmap, a.offsets, a.length};
        q.b[c] = {b.data, b.null_bitmap, b.offsets, b.length};
    }
    if (n == 0) return TSQ_OK;
    q.idx_a = idx_a;
    q.idx_b = idx_b;
    q.n = n;
    q.flags = flags_out;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    hipLaunchKernelGGL(k_rows_equal, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, q);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}
