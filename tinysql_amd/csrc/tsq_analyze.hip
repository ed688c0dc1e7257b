// tsq_analyze.hip — ANALYZE TABLE on device chunks: the column collector (tsq_analyze_*: null / value counts, total size, CM sketch, FM
// sketch, sample) and the histogram of a sorted stream (tsq_sorted_hist_*).  Semantics: include/tsq.h and DESIGN.md "ANALYZE"; the
// scalar core (datum bytes, murmur3, sampling key) is tsq_analyze_dp.h.
//
// Collector.  A push is worked through in SLICES of at most 2^22 rows (from 2^16 rows, doubling, while a sample is taken), one launch of K15a per slice
// over all columns:
//   K15a k_an_collect : a workgroup takes one column after the other.  Per column it clears a private copy of the CM table in LDS
//                       (<= 64 KB), walks its rows (encode in registers, murmur3: the tail path for fixed-width datums, the 16-byte block
//                       loop for strings), updates the LDS counters with LDS atomics and adds the non-zero ones to the table in HBM once.
//                       null / value counts and the total size are reduced per wave.
//        FM sketch    : a hash set in HBM (open addressing, at most half full) holds the hashes that pass the current LEVEL k (k trailing
//                       zero bits); cnt[k] = distinct inserted hashes with at least k trailing zero bits, incremented only by the lane whose
//                       CAS inserted the hash.  For every k >= level all such hashes are inserted, so cnt[k] is exact and the level is
//                       raised only past a k with cnt[k] > max_fm_size: it never overshoots the canonical level.  Between slices the host
//                       reads the state words; when the next slice could fill the set beyond one half, the entries that pass the level
//                       move to a new set (K15b k_an_fm_rebuild).
//        sample       : a non-NULL row with key(r) <= the column's threshold appends (key, ordinal, value) to the candidates (one cursor
//                       add per wave).  When more than 2 * max_sample_size + 4096 candidates are held, the host finds the key of rank
//                       max_sample_size among them (the keys only travel), it becomes the threshold, and K15c keeps the candidates
//                       below it.  The threshold is always a key of rank max_sample_size of the rows seen, so no row of the final sample is
//                       ever dropped.  finish takes the smallest keys and orders them by ordinal.
// Sorted histogram.  finish: K16a flags the run heads (a row that differs from the one before), the positions pass of tsq_compact.h
// ranks them, K16b writes before[j] = the row of head j (= rows before run j), K16c (one wave) walks the buckets: per step one 64-ary
// search in before[] for the last run the bucket absorbs, the bucket table in LDS.
#include "tsq_stage.h"
#include "tsq_compact.h"
#include "tsq_analyze_dp.h"

#include <algorithm>
#include <memory>

#define AN_SLICE_ROWS ((int64_t)1 << 22)
#define AN_FIRST_SLICE_ROWS ((int64_t)1 << 16)
#define AN_ST_WORDS 80
#define AN_ST_NULL 0
#define AN_ST_COUNT 1
#define AN_ST_SIZE 2
#define AN_ST_LEVEL 3
#define AN_ST_LIVE 4
#define AN_ST_ALLONES 5  /* the hash 2^64 - 1 (the set's empty word) was seen at level 0 */
#define AN_ST_SAMPLES 6
#define AN_ST_HEAP 7
#define AN_ST_LOST 8
#define AN_ST_TMP 9
#define AN_ST_CNT 12     /* cnt[0..64] */
#define AN_EMPTY 0xffffffffffffffffULL
#define AN_SAMPLE_SLACK 4096

struct AnCol {
    const void* data;
    const uint8_t* nulls;
    const int64_t* offs;
    int32_t type;
    uint32_t flags;
    unsigned long long* st;
    uint32_t* cm;
    unsigned long long* fm_tab;
    uint64_t fm_cap_mask;
    unsigned long long* s_key;
    unsigned long long* s_ord;
    unsigned long long* s_val;  // the cell's bits, or its offset in the heap
    uint32_t* s_len;
    uint8_t* s_heap;
    uint64_t s_thr;
    uint32_t s_on;
    uint32_t pad;
};
struct AnArgs {
    AnCol col[TSQ_MAX_COLS];
    int32_t n_cols;
    int32_t cm_depth, cm_width, cm_pow2;
    uint32_t wrap;
    int64_t nrows;
    uint64_t row0;  // ordinal of the slice's first row
    uint64_t seed;
    int64_t max_fm;
};

__device__ __forceinline__ void an_fm_insert(const AnCol& k, uint64_t h, int64_t max_fm) {
    unsigned long long* st = k.st;
    const int level = (int)__hip_atomic_load(&st[AN_ST_LEVEL], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
    const int tz = tsq_an_tz(h);
    if (tz < level) return;
    if (h == AN_EMPTY) {
        if (atomicOr(&st[AN_ST_ALLONES], 1ull) & 1ull) return;
    } else {
        uint64_t idx = tsq_mix64(h) & k.fm_cap_mask;
        bool placed = false;
        for (uint64_t step = 0; step <= k.fm_cap_mask; step++) {  // (at most half full: an empty word ends the walk long before)
            unsigned long long s = __hip_atomic_load(&k.fm_tab[idx], __ATOMIC_RELAXED, __HIP_MEMORY_SCOPE_AGENT);
            if (s == h) return;
            if (s == AN_EMPTY) {
                s = atomicCAS(&k.fm_tab[idx], AN_EMPTY, (unsigned long long)h);
                if (s == AN_EMPTY) {
                    placed = true;
                    break;
                }
                if (s == h) return;
            }
            idx = (idx + 1) & k.fm_cap_mask;
        }
        if (!placed) {
            atomicAdd(&st[AN_ST_LOST], 1ull);
            return;
        }
        atomicAdd(&st[AN_ST_LIVE], 1ull);
    }
    for (int j = level; j <= tz; j++) {
        const unsigned long long old = atomicAdd(&st[AN_ST_CNT + j], 1ull);
        if ((int64_t)(old + 1) > max_fm) atomicMax(&st[AN_ST_LEVEL], (unsigned long long)(j + 1));  // (j = 64 holds the hash 0 alone: never raised)
    }
}

__global__ void __launch_bounds__(256) k_an_collect(AnArgs a) {
    extern __shared__ __attribute__((aligned(16))) char an_smem[];
    __shared__ unsigned long long s_red[3][4];
    uint32_t* s_cm = (uint32_t*)an_smem;
    const int tid = threadIdx.x, lane = tid & 63;
    const int ncm = a.cm_depth * a.cm_width;
    const int64_t stride = (int64_t)gridDim.x * 256;
    for (int c = 0; c < a.n_cols; c++) {
        const AnCol& k = a.col[c];
        if (ncm) {
            for (int i = tid; i < ncm; i += 256) s_cm[i] = 0;
            __syncthreads();
        }
        const bool comparable = (k.flags & TSQ_ENC_COMPARABLE) != 0, raw = (k.flags & TSQ_AN_RAW) != 0;
        unsigned long long n_null = 0, n_cnt = 0;
        long long n_size = 0;
        for (int64_t base = (int64_t)blockIdx.x * 256; base < a.nrows; base += stride) {
            const int64_t r = base + tid;
            const bool in = r < a.nrows;
            const bool notnull = in && !tsq_is_null(k.nulls, r);
            n_null += (in && !notnull) ? 1u : 0u;
            bool cand = false;
            uint64_t key = 0, val = 0;
            uint32_t vlen = 0;
            const uint8_t* vsrc = nullptr;
            if (notnull) {
                tsq_mm3 m;
                uint64_t fh, elen;
                if (k.type == TSQ_BYTES) {
                    const int64_t o = k.offs[r];
                    const uint64_t n = (uint64_t)(k.offs[r + 1] - o);
                    vsrc = (const uint8_t*)k.data + o;
                    vlen = (uint32_t)n;
                    const tsq_an_bytes e = tsq_an_cell(vsrc, n, raw, comparable);
                    m = tsq_an_hash(e);
                    elen = tsq_an_len(e);
                    fh = a.wrap ? tsq_an_hash(tsq_an_wrap(e)).h1 : m.h1;
                } else {
                    uint64_t bits;
                    if (k.type == TSQ_F32) {
                        val = ((const uint32_t*)k.data)[r];
                        bits = tsq_f64_bits((double)tsq_bits_f32((uint32_t)val));
                    } else {
                        val = bits = ((const uint64_t*)k.data)[r];
                    }
                    uint64_t lo;
                    uint32_t hi;
                    const uint32_t len = tsq_enc_bytes(k.type, comparable, bits, true, &lo, &hi);
                    m = tsq_mm3_short(lo, hi, len);
                    elen = len;
                    fh = a.wrap ? tsq_an_hash_fixed_wrapped(lo, hi, len).h1 : m.h1;
                }
                n_cnt++;
                n_size += (long long)elen - 1;
                for (int i = 0; i < a.cm_depth; i++) {
                    const uint64_t x = m.h1 + m.h2 * (uint64_t)i;
                    const uint32_t at = a.cm_pow2 ? (uint32_t)(x & (uint64_t)(a.cm_width - 1)) : (uint32_t)(x % (uint64_t)a.cm_width);
                    atomicAdd(&s_cm[i * a.cm_width + at], 1u);
                }
                an_fm_insert(k, fh, a.max_fm);
                if (k.s_on) {
                    key = tsq_an_sample_key(a.seed, a.row0 + (uint64_t)r);
                    cand = key <= k.s_thr;
                }
            }
            const unsigned long long bal = __ballot(cand);
            if (bal) {
                const int leader = __builtin_ffsll((long long)bal) - 1;
                unsigned long long first = 0;
                if (lane == leader) first = atomicAdd(&k.st[AN_ST_SAMPLES], (unsigned long long)__popcll(bal));
                first = __shfl(first, leader, 64);
                if (cand) {
                    const unsigned long long pos = first + __popcll(bal & ((1ull << lane) - 1ull));
                    if (k.type == TSQ_BYTES) {
                        val = atomicAdd(&k.st[AN_ST_HEAP], (unsigned long long)vlen);
                        for (uint32_t i = 0; i < vlen; i++) k.s_heap[val + i] = vsrc[i];
                        k.s_len[pos] = vlen;
                    }
                    k.s_key[pos] = key;
                    k.s_ord[pos] = a.row0 + (uint64_t)r;
                    k.s_val[pos] = val;
                }
            }
        }
        for (int o = 32; o > 0; o >>= 1) {
            n_null += __shfl_xor(n_null, o, 64);
            n_cnt += __shfl_xor(n_cnt, o, 64);
            n_size += __shfl_xor(n_size, o, 64);
        }
        if (lane == 0) {
            s_red[0][tid >> 6] = n_null;
            s_red[1][tid >> 6] = n_cnt;
            s_red[2][tid >> 6] = (unsigned long long)n_size;
        }
        __syncthreads();
        if (tid < 3) {  // one add per workgroup and counter: thousands of waves on three words would queue up in L2
            const unsigned long long v = s_red[tid][0] + s_red[tid][1] + s_red[tid][2] + s_red[tid][3];
            if (v) atomicAdd(&k.st[tid == 0 ? AN_ST_NULL : (tid == 1 ? AN_ST_COUNT : AN_ST_SIZE)], v);
        }
        if (ncm) {
            for (int i = tid; i < ncm; i += 256) {
                const uint32_t v = s_cm[i];
                if (v) atomicAdd(&k.cm[i], v);
            }
        }
        __syncthreads();  // (the next column clears the table and reuses s_red)
    }
}

// the entries of the old set that pass `level` -> an empty set (the hashes are distinct: no comparison)
__global__ void __launch_bounds__(256) k_an_fm_rebuild(const unsigned long long* old_tab, uint64_t old_cap, unsigned long long* tab, uint64_t cap_mask, int level,
                                                       unsigned long long* st) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)old_cap; i += stride) {
        const unsigned long long h = old_tab[i];
        if (h == AN_EMPTY || tsq_an_tz(h) < level) continue;
        uint64_t idx = tsq_mix64(h) & cap_mask;
        bool placed = false;
        for (uint64_t step = 0; step <= cap_mask && !placed; step++) {
            placed = atomicCAS(&tab[idx], AN_EMPTY, h) == AN_EMPTY;
            idx = (idx + 1) & cap_mask;
        }
        if (placed) atomicAdd(&st[AN_ST_LIVE], 1ull);
        else atomicAdd(&st[AN_ST_LOST], 1ull);
    }
}
// the entries that pass `level`, in any order; out holds `out_cap` of them
__global__ void __launch_bounds__(256) k_an_fm_gather(const unsigned long long* tab, uint64_t cap, int level, unsigned long long* out, uint64_t out_cap,
                                                      unsigned long long* st) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < (int64_t)cap; i += stride) {
        const unsigned long long h = tab[i];
        if (h == AN_EMPTY || tsq_an_tz(h) < level) continue;
        const unsigned long long pos = atomicAdd(&st[AN_ST_TMP], 1ull);
        if (pos < out_cap) out[pos] = h;
    }
}
// K15c: the candidates with key <= thr, in any order (finish orders the sample)
struct AnFilterArgs {
    const unsigned long long *key, *ord, *val;
    const uint32_t* len;
    unsigned long long *okey, *oord, *oval;
    uint32_t* olen;
    int64_t n;
    uint64_t thr;
    unsigned long long* st;
    uint64_t out_cap;
};
__global__ void __launch_bounds__(256) k_an_sample_filter(AnFilterArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += stride) {
        const unsigned long long key = a.key[i];
        if (key > a.thr) continue;
        const unsigned long long pos = atomicAdd(&a.st[AN_ST_TMP], 1ull);
        if (pos >= a.out_cap) continue;
        a.okey[pos] = key;
        a.oord[pos] = a.ord[i];
        a.oval[pos] = a.val[i];
        if (a.len) a.olen[pos] = a.len[i];
    }
}

struct AnSampleBufs {
    DevBuf key, ord, val, len;
    int64_t cap = 0;
    void release() {
        for (DevBuf* b : {&key, &ord, &val, &len}) b->release();
        cap = 0;
    }
};
struct AnColHost {
    DevBuf cm, fm_tab, heap, fm_out;
    uint64_t fm_cap = 0;
    AnSampleBufs s[2];
    int cur = 0;
    uint64_t thr = AN_EMPTY;
    // results (finish)
    int64_t null_count = 0, count = 0, total_size = 0;
    uint64_t fm_mask = 0;
    std::vector<uint64_t> fm;
    std::vector<uint32_t> cmv;
    std::vector<uint64_t> s_ord, s_val;
    std::vector<uint32_t> s_len;
    std::vector<uint8_t> s_bytes;  // the sample's cells back to back (TSQ_BYTES)
};

struct tsq_analyze {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    tsq_analyze_cfg cfg;
    std::atomic<int> cancelled{0};
    bool finished = false;
    DevBuf state;           // n_cols x AN_ST_WORDS
    PinnedBuf hstate;       // its copy after every slice
    std::vector<AnColHost> cols;
    std::vector<ColStore> stage;  // host pushes: the chunk in HBM
    DevBuf tmp_bits, tmp_offs;
    DevEvent ev0, ev1;
    int64_t rows = 0;
    double kernel_ms = 0;
    const uint64_t* hst(int c) const { return (const uint64_t*)hstate.p + (size_t)c * AN_ST_WORDS; }
    unsigned long long* dst(int c) const { return state.as<unsigned long long>() + (size_t)c * AN_ST_WORDS; }
};

namespace {

tsq_status an_cancelled(tsq_analyze* a) {
    if (a->cancelled.load()) return tsq_fail(&a->hdr, TSQ_ERR_CANCELLED, "analyze cancelled");
    return TSQ_OK;
}

tsq_status an_read_state(tsq_analyze* a) {
    TSQ_HIP(&a->hdr, hipMemcpyAsync(a->hstate.p, a->state.p, (size_t)a->cfg.n_cols * AN_ST_WORDS * 8, hipMemcpyDeviceToHost, a->ctx->stream));
    TSQ_HIP(&a->hdr, hipStreamSynchronize(a->ctx->stream));
    for (int c = 0; c < a->cfg.n_cols; c++)
        if (a->hst(c)[AN_ST_LOST]) return tsq_fail(&a->hdr, TSQ_ERR_HIP, "tsq_analyze: a walk through the FM hash set found no slot");
    return TSQ_OK;
}

// room for n more hashes in column c's set: at most half full after them
tsq_status an_fm_room(tsq_analyze* a, int c, int64_t n) {
    tsq_ctx* ctx = a->ctx;
    tsq_handle_hdr* h = &a->hdr;
    AnColHost& k = a->cols[c];
    const uint64_t* st = a->hst(c);
    if (k.fm_cap && (st[AN_ST_LIVE] + (uint64_t)n) * 2 <= k.fm_cap) return TSQ_OK;
    const int level = (int)st[AN_ST_LEVEL];
    const uint64_t keep = k.fm_cap ? st[AN_ST_CNT + level] : 0;  // exact: the entries that pass the level
    uint64_t cap = 1024;
    while (cap < 2 * (keep + (uint64_t)n)) cap <<= 1;
    DevBuf nt;
    TSQ_TRY(nt.reserve(ctx, h, (size_t)cap * 8));
    hipError_t e = hipMemsetAsync(nt.p, 0xff, (size_t)cap * 8, ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a->dst(c) + AN_ST_LIVE, 0, 8, ctx->stream);
    if (e == hipSuccess && k.fm_cap) {
        hipLaunchKernelGGL(k_an_fm_rebuild, dim3(tsq_grid_for(ctx, (int64_t)k.fm_cap, 256)), dim3(256), 0, ctx->stream, k.fm_tab.as<unsigned long long>(), k.fm_cap,
                           nt.as<unsigned long long>(), cap - 1, level, a->dst(c));
        e = hipGetLastError();
    }
    if (e != hipSuccess) return tsq_fail(h, TSQ_ERR_HIP, hipGetErrorString(e));
    k.fm_tab = std::move(nt);  // (stream order protects the old set: DevBuf's pool rule)
    k.fm_cap = cap;
    ((uint64_t*)a->hstate.p)[(size_t)c * AN_ST_WORDS + AN_ST_LIVE] = keep;  // (an upper bound until the next read)
    return TSQ_OK;
}

tsq_status an_sample_reserve(tsq_analyze* a, int c, AnSampleBufs& b, int64_t want, int64_t used) {
    tsq_ctx* ctx = a->ctx;
    tsq_handle_hdr* h = &a->hdr;
    if (want <= b.cap) return TSQ_OK;
    const int64_t ncap = std::max<int64_t>(want, b.cap + b.cap / 2);
    TSQ_TRY(b.key.reserve(ctx, h, (size_t)ncap * 8 + 64, true, (size_t)used * 8));
    TSQ_TRY(b.ord.reserve(ctx, h, (size_t)ncap * 8 + 64, true, (size_t)used * 8));
    TSQ_TRY(b.val.reserve(ctx, h, (size_t)ncap * 8 + 64, true, (size_t)used * 8));
    if (a->cfg.col_types[c] == TSQ_BYTES) TSQ_TRY(b.len.reserve(ctx, h, (size_t)ncap * 4 + 64, true, (size_t)used * 4));
    b.cap = ncap;
    return TSQ_OK;
}

// more than 2 K + slack candidates: the key of rank K among them becomes the threshold, the others leave
tsq_status an_sample_tighten(tsq_analyze* a, int c) {
    tsq_ctx* ctx = a->ctx;
    tsq_handle_hdr* h = &a->hdr;
    AnColHost& k = a->cols[c];
    const int64_t K = a->cfg.max_sample_size;
    const int64_t n = (int64_t)a->hst(c)[AN_ST_SAMPLES];
    if (n <= 2 * K + AN_SAMPLE_SLACK) return TSQ_OK;
    std::vector<uint64_t> keys((size_t)n);
    AnSampleBufs& src = k.s[k.cur];
    AnSampleBufs& dst = k.s[k.cur ^ 1];
    TSQ_HIP(h, hipMemcpyAsync(keys.data(), src.key.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    std::nth_element(keys.begin(), keys.begin() + (K - 1), keys.end());
    k.thr = keys[(size_t)K - 1];
    TSQ_TRY(an_sample_reserve(a, c, dst, K, 0));
    AnFilterArgs f;
    memset(&f, 0, sizeof f);
    f.key = src.key.as<unsigned long long>();
    f.ord = src.ord.as<unsigned long long>();
    f.val = src.val.as<unsigned long long>();
    f.okey = dst.key.as<unsigned long long>();
    f.oord = dst.ord.as<unsigned long long>();
    f.oval = dst.val.as<unsigned long long>();
    if (a->cfg.col_types[c] == TSQ_BYTES) {
        f.len = src.len.as<uint32_t>();
        f.olen = dst.len.as<uint32_t>();
    }
    f.n = n;
    f.thr = k.thr;
    f.st = a->dst(c);
    f.out_cap = (uint64_t)dst.cap;
    TSQ_HIP(h, hipMemsetAsync(f.st + AN_ST_TMP, 0, 8, ctx->stream));
    hipLaunchKernelGGL(k_an_sample_filter, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, f);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipMemcpyAsync(f.st + AN_ST_SAMPLES, f.st + AN_ST_TMP, 8, hipMemcpyDeviceToDevice, ctx->stream));
    ((uint64_t*)a->hstate.p)[(size_t)c * AN_ST_WORDS + AN_ST_SAMPLES] = (uint64_t)K;  // (the keys are distinct: exactly K remain)
    k.cur ^= 1;
    return TSQ_OK;
}

// rows [0, n) of device columns `cols` (already sliced), ordinals row0..
tsq_status an_slice(tsq_analyze* a, const tsq_col* cols, int64_t n, uint64_t row0) {
    tsq_ctx* ctx = a->ctx;
    tsq_handle_hdr* h = &a->hdr;
    const tsq_analyze_cfg& cfg = a->cfg;
    AnArgs args;
    memset(&args, 0, sizeof args);
    args.n_cols = cfg.n_cols;
    args.cm_depth = cfg.cm_depth;
    args.cm_width = cfg.cm_width;
    args.cm_pow2 = cfg.cm_width > 0 && (cfg.cm_width & (cfg.cm_width - 1)) == 0;
    args.wrap = cfg.flags & TSQ_AN_WRAP_BYTES;
    args.nrows = n;
    args.row0 = row0;
    args.seed = cfg.sample_seed;
    args.max_fm = cfg.max_fm_size;
    for (int c = 0; c < cfg.n_cols; c++) {
        AnColHost& k = a->cols[c];
        const bool str = cfg.col_types[c] == TSQ_BYTES;
        TSQ_TRY(an_fm_room(a, c, n));
        const int64_t have = (int64_t)a->hst(c)[AN_ST_SAMPLES];
        if (cfg.max_sample_size > 0) {
            TSQ_TRY(an_sample_reserve(a, c, k.s[k.cur], have + n, have));
            if (str) {  // every cell of the slice may become a candidate
                TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 24, cols[c].offsets, 8, hipMemcpyDeviceToHost, ctx->stream));
                TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 25, cols[c].offsets + n, 8, hipMemcpyDeviceToHost, ctx->stream));
                TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
                const int64_t bytes = (int64_t)ctx->pinned[25] - (int64_t)ctx->pinned[24];
                if (bytes < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_analyze_push: var-len column: offsets must not decrease");
                const size_t used = (size_t)a->hst(c)[AN_ST_HEAP];
                TSQ_TRY(k.heap.reserve(ctx, h, used + (size_t)bytes + 64, true, used));
            }
        }
        AnCol& d = args.col[c];
        d.data = cols[c].data;
        d.nulls = cols[c].null_bitmap;
        d.offs = str ? cols[c].offsets : nullptr;
        d.type = cfg.col_types[c];
        d.flags = cfg.col_flags[c];
        d.st = a->dst(c);
        d.cm = k.cm.as<uint32_t>();
        d.fm_tab = k.fm_tab.as<unsigned long long>();
        d.fm_cap_mask = k.fm_cap - 1;
        const AnSampleBufs& s = k.s[k.cur];
        d.s_key = s.key.as<unsigned long long>();
        d.s_ord = s.ord.as<unsigned long long>();
        d.s_val = s.val.as<unsigned long long>();
        d.s_len = s.len.as<uint32_t>();
        d.s_heap = k.heap.as<uint8_t>();
        d.s_thr = k.thr;
        d.s_on = cfg.max_sample_size > 0 ? 1u : 0u;
    }
    const size_t lds = (size_t)cfg.cm_depth * cfg.cm_width * 4;
    // two workgroups per CU (a 64 KB table each): every workgroup adds its table and its counters to HBM once per column and slice
    const int grid = std::min(tsq_grid_for(ctx, n, 256), ctx->num_cus * 2);
    hipLaunchKernelGGL(k_an_collect, dim3(grid), dim3(256), lds, ctx->stream, args);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(an_read_state(a));
    if (cfg.max_sample_size > 0)
        for (int c = 0; c < cfg.n_cols; c++) TSQ_TRY(an_sample_tighten(a, c));
    return TSQ_OK;
}

void an_release(tsq_analyze* a) {  // finish hands the device memory back before the results are read
    for (auto& k : a->cols) {
        for (DevBuf* b : {&k.cm, &k.fm_tab, &k.heap, &k.fm_out}) b->release();
        k.s[0].release();
        k.s[1].release();
    }
    for (auto& s : a->stage) s.release();
    a->state.release();
    a->tmp_bits.release();
    a->tmp_offs.release();
}

}  // namespace

TSQ_API tsq_status tsq_analyze_create(tsq_ctx* ctx, const tsq_analyze_cfg* cfg, tsq_analyze** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || ctx->hdr.magic != TSQ_MAGIC_CTX || !out || !cfg)
        return tsq_fail(ctx && ctx->hdr.magic == TSQ_MAGIC_CTX ? &ctx->hdr : nullptr, TSQ_ERR_INVALID, "tsq_analyze_create: bad arguments");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (cfg->n_cols < 1 || cfg->n_cols > TSQ_MAX_COLS) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_analyze_create: 1..16 columns");
    for (int c = 0; c < cfg->n_cols; c++) {
        if (cfg->col_types[c] < TSQ_I64 || cfg->col_types[c] > TSQ_BYTES) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_analyze_create: unknown column type");
        if (cfg->col_flags[c] & ~(TSQ_ENC_COMPARABLE | TSQ_AN_RAW)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_analyze_create: unknown column flag");
        if ((cfg->col_flags[c] & TSQ_AN_RAW) && cfg->col_types[c] != TSQ_BYTES) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_analyze_create: a raw column is TSQ_BYTES");
    }
    if (cfg->max_sample_size < 0 || cfg->max_fm_size < 1) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_analyze_create: max_sample_size >= 0 and max_fm_size >= 1");
    if (cfg->cm_depth < 0 || cfg->cm_width < 0 || (cfg->cm_depth == 0) != (cfg->cm_width == 0))
        return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_analyze_create: cm_depth and cm_width are both 0 or both positive");
    if ((int64_t)cfg->cm_depth * cfg->cm_width > TSQ_AN_MAX_CM_COUNTERS)
        return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "tsq_analyze_create: a CM sketch of at most 16384 counters is supported");
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    std::unique_ptr<tsq_analyze> a(new tsq_analyze());
    a->hdr.magic = TSQ_MAGIC_ANALYZE;
    a->ctx = ctx;
    a->cfg = *cfg;
    a->cols.resize(cfg->n_cols);
    a->stage.resize(cfg->n_cols);
    for (int c = 0; c < cfg->n_cols; c++) a->stage[c].type = cfg->col_types[c];
    const size_t st_bytes = (size_t)cfg->n_cols * AN_ST_WORDS * 8, cm_bytes = (size_t)cfg->cm_depth * cfg->cm_width * 4;
    tsq_status s = a->state.reserve(ctx, &a->hdr, st_bytes);
    if (s == TSQ_OK) s = a->hstate.reserve(&a->hdr, st_bytes);
    hipError_t e = hipSuccess;
    if (s == TSQ_OK) {
        memset(a->hstate.p, 0, st_bytes);
        e = hipMemsetAsync(a->state.p, 0, st_bytes, ctx->stream);
        if (e == hipSuccess && cm_bytes > 48 * 1024)
            e = hipFuncSetAttribute((const void*)k_an_collect, hipFuncAttributeMaxDynamicSharedMemorySize, (int)cm_bytes);
    }
    for (int c = 0; s == TSQ_OK && e == hipSuccess && cm_bytes && c < cfg->n_cols; c++) {
        s = a->cols[c].cm.reserve(ctx, &a->hdr, cm_bytes);
        if (s == TSQ_OK) e = hipMemsetAsync(a->cols[c].cm.p, 0, cm_bytes, ctx->stream);
    }
    if (s == TSQ_OK && e == hipSuccess) e = a->ev0.create();
    if (s == TSQ_OK && e == hipSuccess) e = a->ev1.create();
    if (s == TSQ_OK && e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (s == TSQ_OK && e != hipSuccess) s = tsq_fail(&a->hdr, TSQ_ERR_HIP, hipGetErrorString(e));
    if (s != TSQ_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return tsq_fail(ch, s, a->hdr.err);
    }
    *out = a.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_push(tsq_analyze* a, const tsq_col* cols, int32_t n_cols, int64_t nrows) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(a, TSQ_MAGIC_ANALYZE));
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &a->hdr;
    TSQ_TRY(an_cancelled(a));
    if (a->finished) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_analyze_push: after tsq_analyze_finish");
    if (nrows < 0 || (nrows > 0 && !cols)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_analyze_push: bad arguments");
    if (nrows == 0) return TSQ_OK;
    bool is_dev = false;
    TSQ_TRY(tsq_validate_cols(h, cols, n_cols, a->cfg.n_cols, a->cfg.col_types, nrows, &is_dev));
    for (int c = 0; c < n_cols; c++)
        if (cols[c].type == TSQ_BYTES && !cols[c].data && nrows > 0 && is_dev) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_analyze_push: var-len column without data");
    tsq_ctx* ctx = a->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    tsq_col dev[TSQ_MAX_COLS];
    for (int c = 0; c < n_cols; c++) {
        dev[c] = cols[c];
        if (is_dev) continue;
        ColStore& s = a->stage[c];
        s.clear();
        if (cols[c].type == TSQ_BYTES) TSQ_TRY(tsq_col_append_varlen(ctx, h, s, cols[c].data, cols[c].offsets, cols[c].null_bitmap, nrows, false, a->tmp_bits, a->tmp_offs));
        else TSQ_TRY(tsq_col_append(ctx, h, s, cols[c].data, cols[c].null_bitmap, nrows, false, a->tmp_bits));
        dev[c].data = s.data.p;
        dev[c].offsets = cols[c].type == TSQ_BYTES ? s.offs.as<int64_t>() : nullptr;
        dev[c].null_bitmap = s.has_nulls ? s.nulls.as<uint8_t>() : nullptr;
        dev[c].flags = TSQ_COL_DEVICE;
    }
    TSQ_HIP(h, hipEventRecord(a->ev0, ctx->stream));
    for (int64_t off = 0, n = 0; off < nrows; off += n) {
        TSQ_TRY(an_cancelled(a));
        // while a sample is taken the slices start small and double: a slice of no more rows than were seen before it brings about
        // max_sample_size candidates under the current threshold, where a first slice of 2^22 rows would hold all of its rows
        int64_t cap = AN_SLICE_ROWS;
        if (a->cfg.max_sample_size > 0) cap = std::min<int64_t>(cap, std::max<int64_t>(AN_FIRST_SLICE_ROWS, (a->rows + off) & ~(int64_t)63));
        n = std::min<int64_t>(nrows - off, cap);
        tsq_col sl[TSQ_MAX_COLS];
        for (int c = 0; c < n_cols; c++) {  // (off is a multiple of 8: the bitmaps start on a byte)
            sl[c] = dev[c];
            if (dev[c].type == TSQ_BYTES) sl[c].offsets = dev[c].offsets + off;
            else sl[c].data = (char*)dev[c].data + (size_t)off * tsq_elem_size(dev[c].type);
            if (dev[c].null_bitmap) sl[c].null_bitmap = dev[c].null_bitmap + (off >> 3);
        }
        TSQ_TRY(an_slice(a, sl, n, (uint64_t)(a->rows + off)));
    }
    TSQ_HIP(h, hipEventRecord(a->ev1, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, a->ev0, a->ev1) == hipSuccess) a->kernel_ms += ms;
    else (void)hipGetLastError();
    a->rows += nrows;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_finish(tsq_analyze* a) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(a, TSQ_MAGIC_ANALYZE));
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &a->hdr;
    TSQ_TRY(an_cancelled(a));
    if (a->finished) return TSQ_OK;
    tsq_ctx* ctx = a->ctx;
    const tsq_analyze_cfg& cfg = a->cfg;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    TSQ_TRY(an_read_state(a));
    const size_t n_cm = (size_t)cfg.cm_depth * cfg.cm_width;
    for (int c = 0; c < cfg.n_cols; c++) {
        AnColHost& k = a->cols[c];
        const uint64_t* st = a->hst(c);
        k.null_count = (int64_t)st[AN_ST_NULL];
        k.count = (int64_t)st[AN_ST_COUNT];
        k.total_size = (int64_t)st[AN_ST_SIZE];
        // FM: the canonical level = the smallest k with cnt[k] <= max_fm_size (exact from the running level on)
        int level = (int)st[AN_ST_LEVEL];
        while (level < 64 && (int64_t)st[AN_ST_CNT + level] > cfg.max_fm_size) level++;
        k.fm_mask = level >= 64 ? ~0ull : ((1ull << level) - 1ull);
        const uint64_t expect = st[AN_ST_CNT + level];
        const bool all_ones = level == 0 && (st[AN_ST_ALLONES] & 1);
        k.fm.assign((size_t)expect, 0);
        const uint64_t in_set = expect - (all_ones ? 1 : 0);
        if (in_set > 0) {
            TSQ_TRY(k.fm_out.reserve(ctx, h, (size_t)in_set * 8 + 64));
            TSQ_HIP(h, hipMemsetAsync(a->dst(c) + AN_ST_TMP, 0, 8, ctx->stream));
            hipLaunchKernelGGL(k_an_fm_gather, dim3(tsq_grid_for(ctx, (int64_t)k.fm_cap, 256)), dim3(256), 0, ctx->stream, k.fm_tab.as<unsigned long long>(), k.fm_cap,
                               level, k.fm_out.as<unsigned long long>(), in_set, a->dst(c));
            TSQ_HIP(h, hipGetLastError());
            TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 26, a->dst(c) + AN_ST_TMP, 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipMemcpyAsync(k.fm.data(), k.fm_out.p, (size_t)in_set * 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
            if (ctx->pinned[26] != in_set) return tsq_fail(h, TSQ_ERR_HIP, "tsq_analyze_finish: the FM hash set and its counters disagree");
        }
        if (all_ones) k.fm[(size_t)in_set] = AN_EMPTY;
        std::sort(k.fm.begin(), k.fm.end());
        if (n_cm) {
            k.cmv.resize(n_cm);
            TSQ_HIP(h, hipMemcpyAsync(k.cmv.data(), k.cm.p, n_cm * 4, hipMemcpyDeviceToHost, ctx->stream));
        }
        // the sample: the max_sample_size smallest keys among the candidates, in row order
        const int64_t n = (int64_t)st[AN_ST_SAMPLES];
        const bool str = cfg.col_types[c] == TSQ_BYTES;
        std::vector<uint64_t> key((size_t)n), ord((size_t)n), val((size_t)n);
        std::vector<uint32_t> len;
        std::vector<uint8_t> heap;
        if (n > 0) {
            const AnSampleBufs& s = k.s[k.cur];
            TSQ_HIP(h, hipMemcpyAsync(key.data(), s.key.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipMemcpyAsync(ord.data(), s.ord.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipMemcpyAsync(val.data(), s.val.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
            if (str) {
                len.resize((size_t)n);
                heap.resize((size_t)st[AN_ST_HEAP]);
                TSQ_HIP(h, hipMemcpyAsync(len.data(), s.len.p, (size_t)n * 4, hipMemcpyDeviceToHost, ctx->stream));
                if (!heap.empty()) TSQ_HIP(h, hipMemcpyAsync(heap.data(), k.heap.p, heap.size(), hipMemcpyDeviceToHost, ctx->stream));
            }
        }
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        std::vector<int64_t> pick((size_t)n);
        for (int64_t i = 0; i < n; i++) pick[(size_t)i] = i;
        const int64_t K = std::min<int64_t>(cfg.max_sample_size, n);
        if (K < n) std::nth_element(pick.begin(), pick.begin() + K, pick.end(), [&](int64_t x, int64_t y) { return key[(size_t)x] < key[(size_t)y]; });
        pick.resize((size_t)K);
        std::sort(pick.begin(), pick.end(), [&](int64_t x, int64_t y) { return ord[(size_t)x] < ord[(size_t)y]; });
        k.s_ord.clear();
        k.s_val.clear();
        k.s_len.clear();
        k.s_bytes.clear();
        for (int64_t i : pick) {
            k.s_ord.push_back(ord[(size_t)i]);
            if (str) {
                k.s_len.push_back(len[(size_t)i]);
                k.s_bytes.insert(k.s_bytes.end(), heap.begin() + (ptrdiff_t)val[(size_t)i], heap.begin() + (ptrdiff_t)(val[(size_t)i] + len[(size_t)i]));
            } else {
                k.s_val.push_back(val[(size_t)i]);
            }
        }
    }
    an_release(a);
    a->finished = true;
    return TSQ_OK;
}

static tsq_status an_result_col(tsq_analyze* a, int32_t c, const char* who) {
    TSQ_TRY(an_cancelled(a));
    if (!a->finished) return tsq_fail(&a->hdr, TSQ_ERR_INVALID, std::string(who) + ": before tsq_analyze_finish");
    if (c < 0 || c >= a->cfg.n_cols) return tsq_fail(&a->hdr, TSQ_ERR_INVALID, std::string(who) + ": no such column");
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_column(tsq_analyze* a, int32_t c, int64_t* null_count, int64_t* count, int64_t* total_size, uint64_t* fm_mask, int64_t* fm_size,
                                      int64_t* cm_count, int64_t* n_samples) {
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    TSQ_TRY(an_result_col(a, c, "tsq_analyze_column"));
    const AnColHost& k = a->cols[c];
    if (null_count) *null_count = k.null_count;
    if (count) *count = k.count;
    if (total_size) *total_size = k.total_size;
    if (fm_mask) *fm_mask = k.fm_mask;
    if (fm_size) *fm_size = (int64_t)k.fm.size();
    if (cm_count) *cm_count = a->cfg.cm_depth ? k.count : 0;
    if (n_samples) *n_samples = (int64_t)k.s_ord.size();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_fm(tsq_analyze* a, int32_t c, uint64_t* hashes_out, int64_t cap) {
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    TSQ_TRY(an_result_col(a, c, "tsq_analyze_fm"));
    const AnColHost& k = a->cols[c];
    if (cap < (int64_t)k.fm.size() || (!hashes_out && !k.fm.empty())) return tsq_fail(&a->hdr, TSQ_ERR_INVALID, "tsq_analyze_fm: the buffer holds fewer than fm_size hashes");
    if (!k.fm.empty()) memcpy(hashes_out, k.fm.data(), k.fm.size() * 8);
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_cm(tsq_analyze* a, int32_t c, uint32_t* counters_out) {
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    TSQ_TRY(an_result_col(a, c, "tsq_analyze_cm"));
    const AnColHost& k = a->cols[c];
    if (k.cmv.empty() || !counters_out) return tsq_fail(&a->hdr, TSQ_ERR_INVALID, "tsq_analyze_cm: no CM sketch was asked for (or a NULL buffer)");
    memcpy(counters_out, k.cmv.data(), k.cmv.size() * 4);
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_samples_peek(tsq_analyze* a, int32_t c, int64_t* n_samples, int64_t* bytes_out) {
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    TSQ_TRY(an_result_col(a, c, "tsq_analyze_samples_peek"));
    if (n_samples) *n_samples = (int64_t)a->cols[c].s_ord.size();
    if (bytes_out) *bytes_out = (int64_t)a->cols[c].s_bytes.size();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_samples(tsq_analyze* a, int32_t c, tsq_col* out, int64_t* ordinals_out, int64_t cap) {
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    TSQ_TRY(an_result_col(a, c, "tsq_analyze_samples"));
    tsq_handle_hdr* h = &a->hdr;
    const AnColHost& k = a->cols[c];
    const int64_t n = (int64_t)k.s_ord.size();
    const int32_t type = a->cfg.col_types[c];
    if (!out || cap < n) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_analyze_samples: the buffers hold fewer rows than the sample");
    if (out->flags & TSQ_COL_DEVICE) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_analyze_samples: the sample is handed out into host buffers");
    if (n > 0 && (!ordinals_out || (type == TSQ_BYTES ? !out->offsets || (!out->data && !k.s_bytes.empty()) : !out->data)))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_analyze_samples: NULL buffer");
    if (type == TSQ_BYTES) {
        if (out->offsets) out->offsets[0] = 0;
        for (int64_t i = 0; i < n; i++) out->offsets[i + 1] = out->offsets[i] + (int64_t)k.s_len[(size_t)i];
        if (!k.s_bytes.empty()) memcpy(out->data, k.s_bytes.data(), k.s_bytes.size());
    } else if (type == TSQ_F32) {
        for (int64_t i = 0; i < n; i++) ((uint32_t*)out->data)[i] = (uint32_t)k.s_val[(size_t)i];
    } else if (n > 0) {
        memcpy(out->data, k.s_val.data(), (size_t)n * 8);
    }
    if (n > 0) memcpy(ordinals_out, k.s_ord.data(), (size_t)n * 8);
    if (out->null_bitmap) memset(out->null_bitmap, 0xff, tsq_bitmap_bytes(n));
    out->length = n;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_stats(tsq_analyze* a, int64_t* rows, double* kernel_ms) {
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    if (rows) *rows = a->rows;
    if (kernel_ms) *kernel_ms = a->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_analyze_cancel(tsq_analyze* a) {
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return TSQ_ERR_INVALID;
    a->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_analyze_destroy(tsq_analyze* a) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(a, TSQ_MAGIC_ANALYZE));
    if (!a || a->hdr.magic != TSQ_MAGIC_ANALYZE) return;
    (void)hipSetDevice(a->ctx->device);
    (void)hipStreamSynchronize(a->ctx->stream);
    a->hdr.magic = 0;
    delete a;
}

// ================================================================ the histogram of a sorted stream
struct ShArgs {
    const void* data;
    const int64_t* offs;
    int32_t type;
    int64_t nrows;
    uint8_t* flags;
    int64_t rows_per_wave;
    const unsigned long long* wave_base;
    int64_t* before;
};

// K16a: flags[r] = 1 iff row r opens a run (row 0, or a row that differs from the one before it)
__global__ void __launch_bounds__(256) k_sh_heads(ShArgs a) {
    const int64_t stride = (int64_t)gridDim.x * blockDim.x;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.nrows; r += stride) {
        bool head = r == 0;
        if (!head) {
            if (a.type == TSQ_BYTES) {
                const int64_t o0 = a.offs[r - 1], o1 = a.offs[r], o2 = a.offs[r + 1];
                head = (o1 - o0) != (o2 - o1);
                const uint8_t* p = (const uint8_t*)a.data;
                for (int64_t i = 0; !head && i < o2 - o1; i++) head = p[o0 + i] != p[o1 + i];
            } else {
                head = ((const uint64_t*)a.data)[r] != ((const uint64_t*)a.data)[r - 1];
            }
        }
        a.flags[r] = head ? 1 : 0;
    }
}
// K16b: before[j] = the row of head j, in row order (the runs and the walk of k_compact_count)
__global__ void __launch_bounds__(256) k_sh_scatter(ShArgs a) {
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
        if (sel) a.before[pos] = r;
    }
}

// K16c: the bucket walk, one wave.  Bucket b = (cnt: cumulative count, rep: rows of its last run, lo / up: its first / last RUN).
// A bucket with lastNumber L and width v absorbs run j while before[j] <= L + v - 1; a run never splits.
struct ShWalkArgs {
    const int64_t* before;  // n_runs + 1 entries, the last one = rows
    int64_t n_runs;
    int64_t num_buckets;
    int64_t cap;            // buckets the table holds
    int64_t* tab;           // 4 x cap words in HBM, used when cap exceeds the LDS table
    int64_t* out;           // result: 4 x cap words (cnt, rep, lower row, upper row)
    int64_t* meta;          // [0] buckets [1] steps
};
#define SH_LDS_BUCKETS 1024
__global__ void __launch_bounds__(64) k_sh_walk(ShWalkArgs a) {
    __shared__ int64_t s_tab[4 * SH_LDS_BUCKETS];
    const int lane = threadIdx.x;
    int64_t* t = a.cap <= SH_LDS_BUCKETS ? s_tab : a.tab;
    int64_t *cnt = t, *rep = t + a.cap, *lo = t + 2 * a.cap, *up = t + 3 * a.cap;
    const int64_t* before = a.before;
    const int64_t R = a.n_runs;
    int64_t idx = 0, L = 0, v = 1, nb = 0, steps = 0;
    int64_t j = 0;
    bool fresh = true;  // the next run opens bucket idx
    while (j < R) {
        if (!fresh) {
            __syncthreads();
            int64_t cur = cnt[idx];
            if (cur + 1 - L > v) {
                if (idx + 1 == a.num_buckets) {  // mergeBuckets: pairs become one bucket, an odd last one stays
                    if (lane == 0) {
                        int64_t w = 0;
                        for (int64_t i = 0; i + 1 <= idx; i += 2, w++) {
                            cnt[w] = cnt[i + 1];
                            rep[w] = rep[i + 1];
                            lo[w] = lo[i];
                            up[w] = up[i + 1];
                        }
                        if ((idx & 1) == 0) {
                            cnt[w] = cnt[idx];
                            rep[w] = rep[idx];
                            lo[w] = lo[idx];
                            up[w] = up[idx];
                        }
                    }
                    __syncthreads();
                    v *= 2;
                    idx /= 2;
                    nb = idx + 1;
                    L = idx == 0 ? 0 : cnt[idx - 1];
                    cur = cnt[idx];
                }
                if (cur + 1 - L > v) {
                    L = cur;
                    idx++;
                    fresh = true;
                }
            }
        }
        if (idx >= a.cap) break;  // (the host sized the table for every reachable bucket)
        // the last run j2 >= j with before[j2] <= T, among the at most v + 1 runs a bucket of width v can hold
        const int64_t T = L + v - 1;
        int64_t p_lo = j, p_hi = (R - j > v + 1) ? j + v + 1 : R;
        while (p_hi - p_lo > 1) {
            const int64_t step = (p_hi - p_lo + 63) / 64;
            const int64_t p = p_lo + (int64_t)(lane + 1) * step;
            const bool ok = p < p_hi && before[p] <= T;
            const int n_ok = __popcll(__ballot(ok));
            const int64_t n_hi = p_lo + (int64_t)(n_ok + 1) * step;
            p_lo += (int64_t)n_ok * step;
            p_hi = n_hi < p_hi ? n_hi : p_hi;
        }
        steps++;
        const int64_t j2 = p_lo;
        if (lane == 0) {
            if (fresh) lo[idx] = j;
            up[idx] = j2;
            cnt[idx] = before[j2 + 1];
            rep[idx] = before[j2 + 1] - before[j2];
        }
        if (fresh) nb = idx + 1;
        fresh = false;
        j = j2 + 1;
    }
    __syncthreads();
    for (int64_t b = lane; b < nb; b += 64) {
        a.out[b] = cnt[b];
        a.out[a.cap + b] = rep[b];
        a.out[2 * a.cap + b] = before[lo[b]];
        a.out[3 * a.cap + b] = before[up[b]];
    }
    if (lane == 0) {
        a.meta[0] = nb;
        a.meta[1] = steps;
    }
}

// bounds: fixed-width cells by row number; var-len: position + length (a scan makes the lengths offsets)
__global__ void __launch_bounds__(256) k_sh_gather(const void* data, const int64_t* offs, int32_t type, const int64_t* rows, int64_t n, uint64_t* out, int64_t* out_len,
                                                   int64_t* out_pos) {
    const int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x;
    if (i >= n) return;
    const int64_t r = rows[i];
    if (type == TSQ_BYTES) {
        out_pos[i] = offs[r];
        out_len[i] = offs[r + 1] - offs[r];
    } else {
        out[i] = ((const uint64_t*)data)[r];
    }
}

struct tsq_sorted_hist {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    int32_t type = TSQ_I64;
    int64_t num_buckets = 0;
    bool finished = false;
    ColStore store;
    DevBuf tmp_bits, tmp_offs, flags, base, before, tab, out, meta, g_data, g_offs, g_pos, g_bytes, scan_tmp;
    DevEvent ev[3];
    // results
    int64_t n_buckets = 0, ndv = 0, steps = 0;
    std::vector<int64_t> res;  // 4 x n_buckets: counts, repeats, lower rows, upper rows
    std::vector<uint64_t> bound_bits[2];
    std::vector<int64_t> bound_offs[2];
    std::vector<uint8_t> bound_bytes[2];
    double scan_ms = 0, walk_ms = 0;
};

namespace {

tsq_status sh_bounds(tsq_sorted_hist* s, int which) {
    tsq_ctx* ctx = s->ctx;
    tsq_handle_hdr* h = &s->hdr;
    const int64_t n = s->n_buckets;
    const bool str = s->type == TSQ_BYTES;
    const int64_t* rows = s->out.as<int64_t>() + (2 + which) * n;  // (the rows were copied back into s->out densely: see finish)
    TSQ_TRY(s->g_data.reserve(ctx, h, (size_t)n * 8 + 64));
    TSQ_TRY(s->g_offs.reserve(ctx, h, ((size_t)n + 2) * 8 + 64));
    TSQ_TRY(s->g_pos.reserve(ctx, h, (size_t)n * 8 + 64));
    hipLaunchKernelGGL(k_sh_gather, dim3((unsigned)((n + 255) / 256)), dim3(256), 0, ctx->stream, s->store.data.p, s->store.offs.as<int64_t>(), s->type, rows, n,
                       s->g_data.as<uint64_t>(), s->g_offs.as<int64_t>(), s->g_pos.as<int64_t>());
    TSQ_HIP(h, hipGetLastError());
    if (!str) {
        s->bound_bits[which].resize((size_t)n);
        TSQ_HIP(h, hipMemcpyAsync(s->bound_bits[which].data(), s->g_data.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        return TSQ_OK;
    }
    TSQ_TRY(tsq_launch_scan64(ctx, h, s->g_offs.as<int64_t>(), n, s->scan_tmp));
    s->bound_offs[which].resize((size_t)n + 1);
    TSQ_HIP(h, hipMemcpyAsync(s->bound_offs[which].data(), s->g_offs.p, ((size_t)n + 1) * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t total = s->bound_offs[which][(size_t)n];
    s->bound_bytes[which].resize((size_t)total);
    if (total > 0) {
        TSQ_TRY(s->g_bytes.reserve(ctx, h, (size_t)total + 64));
        TSQ_TRY(tsq_launch_var_copy(ctx, h, (const uint8_t*)s->store.data.p, s->g_pos.as<int64_t>(), s->g_offs.as<int64_t>(), n, total, s->g_bytes.as<uint8_t>()));
        TSQ_HIP(h, hipMemcpyAsync(s->bound_bytes[which].data(), s->g_bytes.p, (size_t)total, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    }
    return TSQ_OK;
}

}  // namespace

TSQ_API tsq_status tsq_sorted_hist_create(tsq_ctx* ctx, int32_t col_type, int64_t num_buckets, tsq_sorted_hist** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || ctx->hdr.magic != TSQ_MAGIC_CTX || !out)
        return tsq_fail(ctx && ctx->hdr.magic == TSQ_MAGIC_CTX ? &ctx->hdr : nullptr, TSQ_ERR_INVALID, "tsq_sorted_hist_create: bad arguments");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (col_type != TSQ_I64 && col_type != TSQ_U64 && col_type != TSQ_BYTES) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "tsq_sorted_hist_create: TSQ_I64, TSQ_U64 or TSQ_BYTES");
    if (num_buckets < 1) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_sorted_hist_create: num_buckets must be at least 1");
    if (num_buckets > SH_LDS_BUCKETS) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "tsq_sorted_hist_create: at most 1024 buckets");
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    std::unique_ptr<tsq_sorted_hist> s(new tsq_sorted_hist());
    s->hdr.magic = TSQ_MAGIC_SHIST;
    s->ctx = ctx;
    s->type = col_type;
    s->store.type = col_type;
    s->num_buckets = num_buckets;
    for (auto& e : s->ev)
        if (e.create() != hipSuccess) return tsq_fail(ch, TSQ_ERR_HIP, "tsq_sorted_hist_create: hipEventCreate failed");
    *out = s.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_sorted_hist_push(tsq_sorted_hist* s, const tsq_col* col, int64_t nrows) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(s, TSQ_MAGIC_SHIST));
    if (!s || s->hdr.magic != TSQ_MAGIC_SHIST) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &s->hdr;
    if (s->finished) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_sorted_hist_push: after tsq_sorted_hist_finish");
    if (nrows < 0 || (nrows > 0 && !col)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_sorted_hist_push: bad arguments");
    if (nrows == 0) return TSQ_OK;
    bool is_dev = false;
    TSQ_TRY(tsq_validate_cols(h, col, 1, 1, &s->type, nrows, &is_dev));
    if (s->type == TSQ_BYTES && !col->data) {
        const bool empty = !is_dev && col->offsets[nrows] == col->offsets[0];
        if (!empty) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_sorted_hist_push: var-len column without data");
    }
    tsq_ctx* ctx = s->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    if (s->type == TSQ_BYTES) return tsq_col_append_varlen(ctx, h, s->store, col->data, col->offsets, nullptr, nrows, is_dev, s->tmp_bits, s->tmp_offs);
    return tsq_col_append(ctx, h, s->store, col->data, nullptr, nrows, is_dev, s->tmp_bits);
}

TSQ_API tsq_status tsq_sorted_hist_finish(tsq_sorted_hist* s) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(s, TSQ_MAGIC_SHIST));
    if (!s || s->hdr.magic != TSQ_MAGIC_SHIST) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &s->hdr;
    if (s->finished) return TSQ_OK;
    tsq_ctx* ctx = s->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const int64_t N = s->store.rows;
    if (N == 0) {
        s->finished = true;
        return TSQ_OK;
    }
    ShArgs a;
    memset(&a, 0, sizeof a);
    a.data = s->store.data.p;
    a.offs = s->type == TSQ_BYTES ? s->store.offs.as<int64_t>() : nullptr;
    a.type = s->type;
    a.nrows = N;
    TSQ_TRY(s->flags.reserve(ctx, h, (size_t)N + 64));
    a.flags = s->flags.as<uint8_t>();
    const int grid = tsq_grid_for(ctx, N, 256);
    const int n_runs = grid * 4;
    CompactArgs ca;
    memset(&ca, 0, sizeof ca);
    ca.selected = a.flags;
    ca.nrows = N;
    ca.rows_per_wave = (((N + n_runs - 1) / n_runs) + 63) & ~(int64_t)63;
    TSQ_TRY(s->base.reserve(ctx, h, (size_t)n_runs * 8 + 64));
    ca.block_base = s->base.as<unsigned long long>();
    ca.total = ca.block_base + n_runs;
    TSQ_HIP(h, hipEventRecord(s->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_sh_heads, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_compact_count, dim3(grid), dim3(256), 0, ctx->stream, ca);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, ca.block_base, n_runs, ca.total);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 27, ca.total, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t R = (int64_t)ctx->pinned[27];
    if (R < 1 || R > N) return tsq_fail(h, TSQ_ERR_HIP, "tsq_sorted_hist_finish: the positions pass counted an impossible number of runs");
    TSQ_TRY(s->before.reserve(ctx, h, ((size_t)R + 1) * 8 + 64));
    a.rows_per_wave = ca.rows_per_wave;
    a.wave_base = ca.block_base;
    a.before = s->before.as<int64_t>();
    hipLaunchKernelGGL(k_sh_scatter, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    ctx->pinned[28] = (uint64_t)N;
    TSQ_HIP(h, hipMemcpyAsync(a.before + R, ctx->pinned + 28, 8, hipMemcpyHostToDevice, ctx->stream));
    TSQ_HIP(h, hipEventRecord(s->ev[1], ctx->stream));
    // num_buckets = 1: the builder opens a bucket beyond the one it was asked for and then never merges again (builder.go:73): one
    // bucket per run at the most.  Otherwise the bucket index stays below num_buckets.
    ShWalkArgs w;
    memset(&w, 0, sizeof w);
    w.before = a.before;
    w.n_runs = R;
    w.num_buckets = s->num_buckets;
    w.cap = s->num_buckets == 1 ? R : s->num_buckets;
    TSQ_TRY(s->out.reserve(ctx, h, (size_t)w.cap * 32 + 64));
    TSQ_TRY(s->meta.reserve(ctx, h, 64));
    if (w.cap > SH_LDS_BUCKETS) TSQ_TRY(s->tab.reserve(ctx, h, (size_t)w.cap * 32 + 64));
    w.tab = s->tab.as<int64_t>();
    w.out = s->out.as<int64_t>();
    w.meta = s->meta.as<int64_t>();
    hipLaunchKernelGGL(k_sh_walk, dim3(1), dim3(64), 0, ctx->stream, w);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(s->ev[2], ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 29, w.meta, 16, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t nb = (int64_t)ctx->pinned[29];
    s->steps = (int64_t)ctx->pinned[30];
    if (nb < 1 || nb > w.cap) return tsq_fail(h, TSQ_ERR_HIP, "tsq_sorted_hist_finish: the walk left an impossible number of buckets");
    float ms = 0;
    if (hipEventElapsedTime(&ms, s->ev[0], s->ev[1]) == hipSuccess) s->scan_ms = ms;
    if (hipEventElapsedTime(&ms, s->ev[1], s->ev[2]) == hipSuccess) s->walk_ms = ms;
    (void)hipGetLastError();
    s->res.resize((size_t)nb * 4);
    for (int q = 0; q < 4; q++) TSQ_HIP(h, hipMemcpyAsync(s->res.data() + (size_t)q * nb, w.out + (size_t)q * w.cap, (size_t)nb * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    // the four arrays densely at the front of s->out: the bound gathers read the rows from there
    TSQ_HIP(h, hipMemcpyAsync(s->out.p, s->res.data(), (size_t)nb * 32, hipMemcpyHostToDevice, ctx->stream));
    s->n_buckets = nb;
    s->ndv = R;
    TSQ_TRY(sh_bounds(s, 0));
    TSQ_TRY(sh_bounds(s, 1));
    s->finished = true;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_sorted_hist_peek(tsq_sorted_hist* s, int64_t* n_buckets, int64_t* lower_bytes, int64_t* upper_bytes) {
    if (!s || s->hdr.magic != TSQ_MAGIC_SHIST) return TSQ_ERR_INVALID;
    if (!s->finished) return tsq_fail(&s->hdr, TSQ_ERR_INVALID, "tsq_sorted_hist_peek: before tsq_sorted_hist_finish");
    if (n_buckets) *n_buckets = s->n_buckets;
    if (lower_bytes) *lower_bytes = (int64_t)s->bound_bytes[0].size();
    if (upper_bytes) *upper_bytes = (int64_t)s->bound_bytes[1].size();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_sorted_hist_result(tsq_sorted_hist* s, int64_t* n_buckets, int64_t* count, int64_t* ndv, int64_t* counts, int64_t* repeats, int64_t* lower_rows,
                                          int64_t* upper_rows, tsq_col* lower, tsq_col* upper) {
    if (!s || s->hdr.magic != TSQ_MAGIC_SHIST) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &s->hdr;
    if (!s->finished) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_sorted_hist_result: before tsq_sorted_hist_finish");
    const int64_t nb = s->n_buckets;
    if (n_buckets) *n_buckets = nb;
    if (count) *count = s->store.rows;
    if (ndv) *ndv = s->ndv;
    int64_t* dst[4] = {counts, repeats, lower_rows, upper_rows};
    for (int q = 0; q < 4; q++)
        if (dst[q] && nb > 0) memcpy(dst[q], s->res.data() + (size_t)q * nb, (size_t)nb * 8);
    tsq_col* cols[2] = {lower, upper};
    for (int q = 0; q < 2; q++) {
        tsq_col* o = cols[q];
        if (!o) continue;
        if (o->flags & TSQ_COL_DEVICE) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "tsq_sorted_hist_result: the bounds are handed out into host buffers");
        if (o->length < nb) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_sorted_hist_result: a bounds column holds fewer rows than there are buckets");
        if (nb == 0) continue;
        if (s->type == TSQ_BYTES) {
            if (!o->offsets || (!o->data && !s->bound_bytes[q].empty())) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_sorted_hist_result: NULL buffer");
            memcpy(o->offsets, s->bound_offs[q].data(), ((size_t)nb + 1) * 8);
            if (!s->bound_bytes[q].empty()) memcpy(o->data, s->bound_bytes[q].data(), s->bound_bytes[q].size());
        } else {
            if (!o->data) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_sorted_hist_result: NULL buffer");
            memcpy(o->data, s->bound_bits[q].data(), (size_t)nb * 8);
        }
    }
    return TSQ_OK;
}

TSQ_API tsq_status tsq_sorted_hist_stats(tsq_sorted_hist* s, int64_t* rows, double* scan_ms, double* walk_ms, int64_t* steps) {
    if (!s || s->hdr.magic != TSQ_MAGIC_SHIST) return TSQ_ERR_INVALID;
    if (rows) *rows = s->store.rows;
    if (scan_ms) *scan_ms = s->scan_ms;
    if (walk_ms) *walk_ms = s->walk_ms;
    if (steps) *steps = s->steps;
    return TSQ_OK;
}

TSQ_API void tsq_sorted_hist_destroy(tsq_sorted_hist* s) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(s, TSQ_MAGIC_SHIST));
    if (!s || s->hdr.magic != TSQ_MAGIC_SHIST) return;
    (void)hipSetDevice(s->ctx->device);
    (void)hipStreamSynchronize(s->ctx->stream);
    s->hdr.magic = 0;
    delete s;
}
