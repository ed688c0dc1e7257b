// tsq_membuf.hip — the transaction's write buffer on the GPU (gfx950): kv.memDbBuffer (kv/memdb_buffer.go:95-114) as
// twoPhaseCommitter.initKeysAndMutations walks it (store/tikv/2pc.go:115-172), kept in HBM and turned into a strictly ascending
// tsq_mvcc_write_req (include/tsq.h "Transaction buffer").  The per-key code is tsq_membuf_dp.h.
//
// tsq_membuf_push:
//   K25a k_mb_push     : one lane per row — its offsets, the empty key, the nil value, the entry limit; the entry's place in the
//                        buffer's bytes, its lengths and kind behind the entries that are there
// tsq_membuf_finish:
//   K25b k_mb_survey   : one lane per entry — shortest and longest key, the prefix shared with entry 0 (a min-reduction: bytes in
//                        front of it are never looked at again), "entry e - 1 < entry e" for all e (then no sort runs), the first lock
//        (the host reads the control words)
//   K25c k_mb_iota / k_mb_image : the entry ids in sequence order; then per element of the sort tuple, least significant first (the
//                        tail, then the 8-byte images from the last to the first), the image of every entry in the current order
//                        with the OR and AND of all images: a digit that is the same in every entry is skipped
//   K25d k_mb_tilehist / k_mb_scan_rows / k_mb_scan_totals / k_mb_scatter : one stable radix pass over (image, entry id), 4096
//                        entries per tile, ranks by ballot, no atomics in the scatter (the pass of tsq_sort.hip)
//   K25e k_mb_winner   : one lane per sorted position — the last entry of a run of equal keys survives; tsq_launch_scan64 over the flags
//   K25f k_mb_place    : the survivors' entry id, op and lengths at their final index, the counts and the primary
//        tsq_launch_scan64 x 2: lengths -> offsets (the host reads the byte totals, which size the request's byte arrays)
//   K25g k_mb_copy     : keys, then values, to their final place; a cell of the threshold length (TSQ_KNOB_ROWENC_WAVE_COPY, 64)
//                        or more is copied by the whole wave, as k_rg_copy does
// tsq_membuf_get:
//   K25h k_mb_get      : one lane per probe key — binary search over the request's keys; a lock-only entry is a miss
// Every kernel is a grid-stride loop over rows (tiles for the pass) sized by the row count and capped at 8 workgroups per CU, as
// tsq_grid_for and the passes of tsq_sort.hip do; no kernel assumes n > 0.
#include "tsq_radix.h"
#include "tsq_membuf_store.h"
#include "tsq_membuf_dp.h"

#include <memory>

#define TSQ_MB_NT 256
#define TSQ_MB_K 16
#define TSQ_MB_T (TSQ_MB_NT * TSQ_MB_K)  // entries per tile of a radix pass
#define TSQ_MB_NW (TSQ_MB_NT / 64)
#define TSQ_MB_DEFAULT_WAVE_COPY 64
#define TSQ_MB_NONE (~0ull)

// the words the kernels of one call share and the host reads
struct MbCtl {
    unsigned int err;
    unsigned int unsorted;
    unsigned long long first_error;  // push: the first refused row; NONE
    unsigned long long min_len, max_len, prefix;
    unsigned long long first_lock;   // the lock entry with the smallest sequence number; NONE
    unsigned long long first_put;    // the smallest final index that is not lock-only; NONE
    unsigned long long lock_primary; // the final index of first_lock's key
    unsigned long long puts, dels, locks, size;
    unsigned long long orand[2];
};

struct MbPushArgs {
    tsq_mb_push_view p;
    int64_t base, kbase, vbase;  // entries, key bytes and value bytes that are there
    int64_t* kbeg;
    int64_t* klen;
    int64_t* vbeg;
    int64_t* vlen;
    uint8_t* kind;
    MbCtl* ctl;
};
__global__ void __launch_bounds__(256) k_mb_push(MbPushArgs a) {
    unsigned int ebits = 0;
    unsigned long long first = TSQ_MB_NONE;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.p.n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t kb, kl, vb, vl;
        const uint32_t e = tsq_mb_push_check(a.p, i, &kb, &kl, &vb, &vl);
        if (e) {
            ebits |= e;
            first = (unsigned long long)i < first ? (unsigned long long)i : first;
        } else {
            a.kbeg[a.base + i] = a.kbase + kb;
            a.klen[a.base + i] = kl;
            a.vbeg[a.base + i] = a.vbase + vb;
            a.vlen[a.base + i] = vl;
            a.kind[a.base + i] = (uint8_t)a.p.kind;
        }
    }
    if (ebits) {
        atomicOr(&a.ctl->err, ebits);
        atomicMin(&a.ctl->first_error, first);
    }
}

// the entries (by sequence number) and the sort's buffers
struct MbArgs {
    const uint8_t* keys;
    const int64_t* kbeg;
    const int64_t* klen;
    const int64_t* vlen;
    const uint8_t* kind;
    int64_t n;
    int64_t prefix;
    int64_t depth;  // k_mb_image: the image, -1: the tail
    const uint64_t* img_in;
    const uint32_t* idx_in;
    uint64_t* img_out;
    uint32_t* idx_out;
    int32_t digit;
    int64_t ntiles;
    uint32_t* hist;    // [256][ntiles]
    uint32_t* totals;  // [256]
    MbCtl* ctl;
    // the result
    int64_t* win;      // [n + 1]: the flag, then (scan) the survivors in front of every sorted position
    int32_t* src;      // [m]: the entry behind every final index
    uint8_t* ops;
    int64_t* okoff;    // [m + 1]: lengths, then (scan) offsets
    int64_t* ovoff;
};

__global__ void __launch_bounds__(256) k_mb_survey(MbArgs a) {
    unsigned long long mn = TSQ_MB_NONE, mx = 0, pf = TSQ_MB_NONE, fl = TSQ_MB_NONE;
    unsigned int uns = 0;
    for (int64_t e = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; e < a.n; e += (int64_t)gridDim.x * blockDim.x) {
        const unsigned long long len = (unsigned long long)a.klen[e];
        mn = len < mn ? len : mn;
        mx = len > mx ? len : mx;
        const unsigned long long c = (unsigned long long)tsq_mb_common_prefix(a.keys + a.kbeg[0], a.klen[0], a.keys + a.kbeg[e], a.klen[e], a.klen[0]);
        pf = c < pf ? c : pf;
        if (e > 0 && !tsq_mb_ascending_at(a.keys, a.kbeg, a.klen, e)) uns = 1;
        if (a.kind[e] == TSQ_MEMBUF_LOCK && (unsigned long long)e < fl) fl = (unsigned long long)e;
    }
    for (int o = 32; o > 0; o >>= 1) {
        unsigned long long y = __shfl_xor(mn, o, 64);
        mn = y < mn ? y : mn;
        y = __shfl_xor(mx, o, 64);
        mx = y > mx ? y : mx;
        y = __shfl_xor(pf, o, 64);
        pf = y < pf ? y : pf;
        y = __shfl_xor(fl, o, 64);
        fl = y < fl ? y : fl;
        uns |= __shfl_xor(uns, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (mn != TSQ_MB_NONE) atomicMin(&a.ctl->min_len, mn);
        if (mx) atomicMax(&a.ctl->max_len, mx);
        if (pf != TSQ_MB_NONE) atomicMin(&a.ctl->prefix, pf);
        if (fl != TSQ_MB_NONE) atomicMin(&a.ctl->first_lock, fl);
        if (uns) atomicOr(&a.ctl->unsorted, 1u);
    }
}

__global__ void __launch_bounds__(256) k_mb_iota(uint32_t* idx, int64_t n) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < n; i += (int64_t)gridDim.x * blockDim.x) idx[i] = (uint32_t)i;
}

// the image of the entry at every position of the current order, and the OR / AND of all of them
__global__ void __launch_bounds__(256) k_mb_image(MbArgs a) {
    unsigned long long vor = 0, vand = ~0ull;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const uint32_t e = a.idx_in[i];
        uint64_t v = 0;
        if ((int64_t)e < a.n)  // (an entry id is below n: checked, not assumed)
            v = a.depth < 0 ? tsq_mb_tail_image(a.klen[e], a.prefix, a.kind[e]) : tsq_mb_image(a.keys + a.kbeg[e], a.klen[e], a.prefix, a.depth);
        a.img_out[i] = v;
        vor |= v;
        vand &= v;
    }
    for (int o = 32; o; o >>= 1) {
        vor |= __shfl_xor(vor, o, 64);
        vand &= __shfl_xor(vand, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        atomicOr(&a.ctl->orand[0], vor);
        atomicAnd(&a.ctl->orand[1], vand);
    }
}

__device__ __forceinline__ uint32_t mb_digit(const MbArgs& a, uint64_t img) { return (uint32_t)(img >> (8 * a.digit)) & 255u; }

__global__ void __launch_bounds__(TSQ_MB_NT) k_mb_tilehist(MbArgs a) {
    __shared__ uint32_t s_h[256];
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        s_h[threadIdx.x] = 0;
        __syncthreads();
        const int64_t base = t * TSQ_MB_T;
#pragma unroll 4
        for (int j = 0; j < TSQ_MB_K; j++) {
            const int64_t i = base + (int64_t)j * TSQ_MB_NT + threadIdx.x;
            if (i < a.n) atomicAdd(&s_h[mb_digit(a, a.img_in[i])], 1u);
        }
        __syncthreads();
        a.hist[(int64_t)threadIdx.x * a.ntiles + t] = s_h[threadIdx.x];
        __syncthreads();
    }
}
// workgroup d: exclusive scan of hist[d][0..ntiles) in place, totals[d] = row sum
__global__ void __launch_bounds__(1024) k_mb_scan_rows(MbArgs a) {
    __shared__ uint32_t s_wsum[16];
    uint32_t* row = a.hist + (int64_t)blockIdx.x * a.ntiles;
    uint32_t carry = 0;
    for (int64_t c0 = 0; c0 < a.ntiles; c0 += 1024) {
        const int64_t i = c0 + threadIdx.x;
        const uint32_t v = i < a.ntiles ? row[i] : 0u;
        uint32_t total;
        const uint32_t ex = block_excl_scan<1024>(v, s_wsum, &total);
        if (i < a.ntiles) row[i] = carry + ex;
        carry += total;
        __syncthreads();
    }
    if (threadIdx.x == 0) a.totals[blockIdx.x] = carry;
}
__global__ void __launch_bounds__(256) k_mb_scan_totals(MbArgs a) {
    __shared__ uint32_t s_wsum[4];
    uint32_t total;
    const uint32_t ex = block_excl_scan<256>(a.totals[threadIdx.x], s_wsum, &total);
    a.totals[threadIdx.x] = ex;
}
// stable ranks without atomics: every wave owns a contiguous quarter of the tile, matches equal digits with 8 ballots and keeps its
// running digit counts in LDS; the tile is laid out sorted in LDS and every digit run is written by consecutive lanes
__global__ void __launch_bounds__(TSQ_MB_NT) k_mb_scatter(MbArgs a) {
    __shared__ uint64_t s_img[TSQ_MB_T];
    __shared__ uint32_t s_idx[TSQ_MB_T];
    __shared__ uint32_t s_whist[TSQ_MB_NW][256];
    __shared__ uint32_t s_start[256];
    __shared__ uint32_t s_gbase[256];
    __shared__ uint32_t s_wsum[TSQ_MB_NT / 64];
    const uint32_t tid = threadIdx.x, lane = tid & 63u, w = tid >> 6;
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t t = blockIdx.x; t < a.ntiles; t += gridDim.x) {
        const int64_t base = t * TSQ_MB_T;
#pragma unroll
        for (int q = 0; q < TSQ_MB_NW; q++) s_whist[q][tid] = 0;
        s_gbase[tid] = a.totals[tid] + a.hist[(int64_t)tid * a.ntiles + t];
        __syncthreads();
        uint64_t img[TSQ_MB_K];
        uint32_t idx[TSQ_MB_K], rk[TSQ_MB_K];  // rk = digit << 16 | rank inside the wave's quarter
#pragma unroll
        for (int j = 0; j < TSQ_MB_K; j++) {
            const int64_t i = base + (int64_t)w * (64 * TSQ_MB_K) + j * 64 + lane;
            const bool ok = i < a.n;
            img[j] = ok ? a.img_in[i] : 0ull;
            idx[j] = ok ? a.idx_in[i] : 0u;
        }
#pragma unroll
        for (int j = 0; j < TSQ_MB_K; j++) {
            const int64_t i = base + (int64_t)w * (64 * TSQ_MB_K) + j * 64 + lane;
            const bool ok = i < a.n;
            const uint32_t d = ok ? mb_digit(a, img[j]) : 0u;
            unsigned long long peers = __ballot(ok);
#pragma unroll
            for (int b = 0; b < 8; b++) {
                const unsigned long long bal = __ballot((d >> b) & 1u);
                peers &= ((d >> b) & 1u) ? bal : ~bal;
            }
            const uint32_t before = (uint32_t)__popcll(peers & lt);
            const uint32_t prev = s_whist[w][d];  // every lane of the match group reads before its first lane adds
            if (ok && before == 0) s_whist[w][d] = prev + (uint32_t)__popcll(peers);
            rk[j] = ok ? ((d << 16) | (prev + before)) : 0xffffffffu;
        }
        __syncthreads();
        {
            uint32_t run = 0;
#pragma unroll
            for (int q = 0; q < TSQ_MB_NW; q++) {
                const uint32_t c = s_whist[q][tid];
                s_whist[q][tid] = run;
                run += c;
            }
            uint32_t total;
            s_start[tid] = block_excl_scan<TSQ_MB_NT>(run, s_wsum, &total);
        }
        __syncthreads();
#pragma unroll
        for (int j = 0; j < TSQ_MB_K; j++) {
            if (rk[j] != 0xffffffffu) {
                const uint32_t d = rk[j] >> 16;
                const uint32_t pos = s_start[d] + s_whist[w][d] + (rk[j] & 0xffffu);  // (< the tile's entries <= TSQ_MB_T)
                s_img[pos] = img[j];
                s_idx[pos] = idx[j];
            }
        }
        __syncthreads();
        const int64_t left = a.n - base;
        const uint32_t nt = left < TSQ_MB_T ? (uint32_t)left : (uint32_t)TSQ_MB_T;
        for (uint32_t i = tid; i < nt; i += TSQ_MB_NT) {
            const uint64_t v = s_img[i];
            const uint32_t d = mb_digit(a, v);
            const int64_t dst = (int64_t)s_gbase[d] + (i - s_start[d]);
            if (dst < a.n) {  // (the histogram's ranks stay below n: checked, not assumed)
                a.img_out[dst] = v;
                a.idx_out[dst] = s_idx[i];
            }
        }
        __syncthreads();
    }
}

__global__ void __launch_bounds__(256) k_mb_winner(MbArgs a) {
    tsq_mb_sorted s;
    s.keys = a.keys, s.kbeg = a.kbeg, s.klen = a.klen, s.order = a.idx_in, s.n = a.n, s.prefix = a.prefix;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const bool ok = (int64_t)a.idx_in[i] < a.n && (i + 1 >= a.n || (int64_t)a.idx_in[i + 1] < a.n);
        a.win[i] = ok && tsq_mb_is_winner(s, i) ? 1 : 0;
    }
}

__global__ void __launch_bounds__(256) k_mb_place(MbArgs a) {
    unsigned long long puts = 0, dels = 0, locks = 0, size = 0, fp = TSQ_MB_NONE;
    const int64_t m = a.win[a.n];
    const unsigned long long first_lock = a.ctl->first_lock;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = a.win[i];
        const uint32_t e = a.idx_in[i];
        if (o < 0 || o >= m || (int64_t)e >= a.n) continue;  // (the scan of n flags stays below their sum)
        if ((unsigned long long)e == first_lock) a.ctl->lock_primary = (unsigned long long)o;  // (one entry has that id: one writer)
        if (a.win[i + 1] == o) continue;
        const uint8_t k = a.kind[e];
        a.src[o] = (int32_t)e;
        a.ops[o] = k;  // TSQ_MEMBUF_SET / DELETE / LOCK are TSQ_MVCC_OP_PUT / DEL / LOCK
        a.okoff[o] = a.klen[e];
        a.ovoff[o] = k == TSQ_MEMBUF_SET ? a.vlen[e] : 0;
        size += (unsigned long long)a.klen[e] + (k == TSQ_MEMBUF_SET ? (unsigned long long)a.vlen[e] : 0ull);
        if (k == TSQ_MEMBUF_SET) puts++;
        else if (k == TSQ_MEMBUF_DELETE) dels++;
        else locks++;
        if (k != TSQ_MEMBUF_LOCK && (unsigned long long)o < fp) fp = (unsigned long long)o;
    }
    for (int o = 32; o > 0; o >>= 1) {
        puts += __shfl_xor(puts, o, 64);
        dels += __shfl_xor(dels, o, 64);
        locks += __shfl_xor(locks, o, 64);
        size += __shfl_xor(size, o, 64);
        const unsigned long long y = __shfl_xor(fp, o, 64);
        fp = y < fp ? y : fp;
    }
    if ((threadIdx.x & 63) == 0) {
        if (puts) atomicAdd(&a.ctl->puts, puts);
        if (dels) atomicAdd(&a.ctl->dels, dels);
        if (locks) atomicAdd(&a.ctl->locks, locks);
        if (size) atomicAdd(&a.ctl->size, size);
        if (fp != TSQ_MB_NONE) atomicMin(&a.ctl->first_put, fp);
    }
}

// cell o of the result: doff[o + 1] - doff[o] bytes from sbeg[src[o]] of the buffer's bytes
struct MbCopyArgs {
    const uint8_t* sbytes;
    const int64_t* sbeg;
    const int32_t* src;
    uint8_t* dst;
    const int64_t* doff;
    int64_t m;
    int64_t n;          // entries: src[o] < n
    int64_t src_bytes;  // sbeg[e] + length <= src_bytes
    int64_t dst_bytes;
    int64_t wave_copy;
};
__global__ void __launch_bounds__(256) k_mb_copy(MbCopyArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r0 = wave * 64; r0 < a.m; r0 += nwaves * 64) {  // (wave uniform)
        const int64_t o = r0 + lane;
        int64_t len = 0;
        const uint8_t* s = a.sbytes;
        uint8_t* d = a.dst;
        if (o < a.m) {
            const int64_t o0 = a.doff[o], e = a.src[o];
            len = a.doff[o + 1] - o0;
            if (len > 0 && e >= 0 && e < a.n && o0 >= 0 && o0 + len <= a.dst_bytes && a.sbeg[e] >= 0 && a.sbeg[e] + len <= a.src_bytes) {
                d = a.dst + o0;
                s = a.sbytes + a.sbeg[e];
            } else {
                len = 0;
            }
        }
        const bool by_wave = a.wave_copy > 0 && len >= a.wave_copy;
        if (len > 0 && !by_wave) tsq_copy_cell(d, s, len);
        unsigned long long todo = __ballot(by_wave);
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

struct MbGetArgs {
    const uint8_t* okeys;
    const int64_t* okoff;
    const uint8_t* oops;  // a lock-only entry is not in the reference's buffer: a miss
    int64_t m;
    const uint8_t* pkeys;
    const int64_t* pkoff;  // or NULL: fixed_len
    int64_t fixed_len;
    int64_t pkey_bytes;
    int64_t n;
    int64_t* out;
    MbCtl* ctl;
};
__global__ void __launch_bounds__(256) k_mb_get(MbGetArgs a) {
    unsigned int e = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t b, len;
        if (a.pkoff) {
            if (!tsq_mb_pair_ok(a.pkoff, i, a.pkey_bytes)) {
                e |= TSQ_MB_E_OFFSETS;
                a.out[i] = -1;
                continue;
            }
            b = a.pkoff[i], len = a.pkoff[i + 1] - b;
        } else {
            b = i * a.fixed_len, len = a.fixed_len;
            if (len < 0 || b + len > a.pkey_bytes) {
                e |= TSQ_MB_E_OFFSETS;
                a.out[i] = -1;
                continue;
            }
        }
        const int64_t at = tsq_mb_find(a.okeys, a.okoff, a.m, a.pkeys + b, len);
        a.out[i] = at >= 0 && a.oops[at] == TSQ_MVCC_OP_LOCK ? -1 : at;
    }
    if (e) atomicOr(&a.ctl->err, e);
}

// ====================================================================== host side
namespace {
const char* mb_push_message(unsigned int e) {
    if (e & TSQ_MB_E_OFFSETS) return "membuf: offsets decrease or leave their buffer";
    if (e & TSQ_MB_E_EMPTY_KEY) return "membuf: empty key";
    if (e & TSQ_MB_E_NIL_VALUE) return "membuf: cannot set nil value";
    return "membuf: entry too large";
}

tsq_status mb_copy_in(tsq_ctx* ctx, tsq_handle_hdr* h, void* dst, const void* src, size_t bytes, bool dev) {
    if (bytes) TSQ_HIP(h, hipMemcpyAsync(dst, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return TSQ_OK;
}

tsq_status mb_ctl_reset(tsq_membuf* mb, MbCtl* host) {
    tsq_ctx* ctx = mb->ctx;
    memset(host, 0, sizeof *host);
    host->first_error = host->min_len = host->prefix = host->first_lock = host->first_put = host->lock_primary = TSQ_MB_NONE;
    host->orand[1] = ~0ull;
    TSQ_TRY(mb->ctl.reserve(ctx, &mb->hdr, sizeof(MbCtl) + 64));
    TSQ_HIP(&mb->hdr, hipMemcpyAsync(mb->ctl.p, host, sizeof *host, hipMemcpyHostToDevice, ctx->stream));
    TSQ_HIP(&mb->hdr, hipStreamSynchronize(ctx->stream));  // (host is the caller's local: the copy has left it)
    return TSQ_OK;
}
tsq_status mb_ctl_read(tsq_membuf* mb, MbCtl* host) {
    TSQ_HIP(&mb->hdr, hipMemcpyAsync(host, mb->ctl.p, sizeof *host, hipMemcpyDeviceToHost, mb->ctx->stream));
    TSQ_HIP(&mb->hdr, hipStreamSynchronize(mb->ctx->stream));
    return TSQ_OK;
}

// the probe keys or a push's offsets on the device: the caller's own array, or a copy in tmp
tsq_status mb_dev_array(tsq_ctx* ctx, tsq_handle_hdr* h, DevBuf& tmp, const void* src, size_t bytes, bool dev, const void** out) {
    *out = src;
    if (dev || !src) return TSQ_OK;
    TSQ_TRY(tmp.reserve(ctx, h, bytes + 64));
    TSQ_TRY(mb_copy_in(ctx, h, tmp.p, src, bytes, false));
    *out = tmp.p;
    return TSQ_OK;
}

// one stable radix pass on digit `digit` of the images: (img_in, idx_in) -> (img_out, idx_out)
tsq_status mb_pass(tsq_membuf* mb, MbArgs& a, int digit) {
    tsq_ctx* ctx = mb->ctx;
    a.digit = digit;
    const int tiles_grid = (int)std::min<int64_t>(a.ntiles, (int64_t)ctx->num_cus * 8);
    hipLaunchKernelGGL(k_mb_tilehist, dim3(tiles_grid), dim3(TSQ_MB_NT), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_mb_scan_rows, dim3(256), dim3(1024), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_mb_scan_totals, dim3(1), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_mb_scatter, dim3(tiles_grid), dim3(TSQ_MB_NT), 0, ctx->stream, a);
    TSQ_HIP(&mb->hdr, hipGetLastError());
    return TSQ_OK;
}

tsq_status mb_finish(tsq_membuf* mb, tsq_membuf_result* result) {
    tsq_handle_hdr* h = &mb->hdr;
    tsq_ctx* ctx = mb->ctx;
    const int64_t n = mb->n;
    mb->finished = false;
    mb->forget_reads();
    mb->m = 0;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    DevBuf img[2], idx[2], hist, totals, win, src, scan_tmp;
    StreamDrain drain(ctx->stream);  // every exit waits for the kernels that use them
    float ms = 0;
    double kernel_ms = 0;
    MbCtl ctl;
    TSQ_TRY(mb_ctl_reset(mb, &ctl));

    MbArgs a;
    memset(&a, 0, sizeof a);
    a.keys = mb->keys.as<uint8_t>();
    a.kbeg = mb->kbeg.as<int64_t>();
    a.klen = mb->klen.as<int64_t>();
    a.vlen = mb->vlen.as<int64_t>();
    a.kind = mb->kind.as<uint8_t>();
    a.n = n;
    a.ctl = mb->ctl.as<MbCtl>();
    const int grid = tsq_grid_for(ctx, n, 256);

    TSQ_HIP(h, hipEventRecord(mb->ev[0], ctx->stream));
    if (n > 0) hipLaunchKernelGGL(k_mb_survey, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(mb->ev[1], ctx->stream));
    TSQ_TRY(mb_ctl_read(mb, &ctl));
    if (hipEventElapsedTime(&ms, mb->ev[0], mb->ev[1]) == hipSuccess) kernel_ms += ms;
    int64_t prefix = 0, depths = 0;
    if (n > 0) {
        if (ctl.min_len == TSQ_MB_NONE || ctl.min_len == 0 || ctl.max_len < ctl.min_len || ctl.prefix > ctl.min_len)
            return tsq_fail(h, TSQ_ERR_HIP, "internal: the key lengths of the transaction buffer are out of range");
        prefix = (int64_t)ctl.prefix;
        depths = tsq_mb_depths((int64_t)ctl.max_len, prefix);
    }
    a.prefix = prefix;

    // ---- the order
    int64_t passes = 0;
    int cur = 0;
    TSQ_TRY(idx[0].reserve(ctx, h, (size_t)n * 4 + 64));
    TSQ_HIP(h, hipEventRecord(mb->ev[0], ctx->stream));
    if (n > 0) hipLaunchKernelGGL(k_mb_iota, dim3(grid), dim3(256), 0, ctx->stream, idx[0].as<uint32_t>(), n);
    TSQ_HIP(h, hipGetLastError());
    if (n > 1 && ctl.unsorted) {
        a.ntiles = (n + TSQ_MB_T - 1) / TSQ_MB_T;
        TSQ_TRY(idx[1].reserve(ctx, h, (size_t)n * 4 + 64));
        TSQ_TRY(img[0].reserve(ctx, h, (size_t)n * 8 + 64));
        TSQ_TRY(img[1].reserve(ctx, h, (size_t)n * 8 + 64));
        TSQ_TRY(hist.reserve(ctx, h, (size_t)a.ntiles * 256 * 4 + 64));
        TSQ_TRY(totals.reserve(ctx, h, 256 * 4 + 64));
        a.hist = hist.as<uint32_t>();
        a.totals = totals.as<uint32_t>();
        for (int64_t d = -1, step = 0; step <= depths; step++, d = depths - step) {  // the tail, then the images from the last to the first
            a.depth = d;
            a.idx_in = idx[cur].as<uint32_t>();
            a.img_out = img[cur].as<uint64_t>();
            const unsigned long long init[2] = {0ull, ~0ull};
            TSQ_HIP(h, hipMemcpyAsync(&a.ctl->orand[0], init, 16, hipMemcpyHostToDevice, ctx->stream));
            hipLaunchKernelGGL(k_mb_image, dim3(grid), dim3(256), 0, ctx->stream, a);
            TSQ_HIP(h, hipGetLastError());
            unsigned long long orand[2] = {0, 0};
            TSQ_HIP(h, hipMemcpyAsync(orand, &a.ctl->orand[0], 16, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
            const unsigned long long differ = orand[0] ^ orand[1];
            for (int digit = 0; digit < 8; digit++) {
                if (!((differ >> (8 * digit)) & 255ull)) continue;  // the same in every entry: the pass would move nothing
                a.img_in = img[cur].as<uint64_t>();
                a.idx_in = idx[cur].as<uint32_t>();
                a.img_out = img[cur ^ 1].as<uint64_t>();
                a.idx_out = idx[cur ^ 1].as<uint32_t>();
                TSQ_TRY(mb_pass(mb, a, digit));
                cur ^= 1;
                passes++;
            }
        }
    }
    a.idx_in = idx[cur].as<uint32_t>();

    // ---- the survivors
    TSQ_TRY(win.reserve(ctx, h, ((size_t)n + 1) * 8 + 64));
    a.win = win.as<int64_t>();
    if (n > 0) hipLaunchKernelGGL(k_mb_winner, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.win, n, scan_tmp));
    int64_t m = 0;
    TSQ_HIP(h, hipMemcpyAsync(&m, a.win + n, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (m < 0 || m > n || (n > 0 && m == 0)) return tsq_fail(h, TSQ_ERR_HIP, "internal: the entry count of the transaction buffer is out of range");
    TSQ_TRY(src.reserve(ctx, h, (size_t)m * 4 + 64));
    TSQ_TRY(mb->oops.reserve(ctx, h, (size_t)m + 64));
    TSQ_TRY(mb->okoff.reserve(ctx, h, ((size_t)m + 1) * 8 + 64));
    TSQ_TRY(mb->ovoff.reserve(ctx, h, ((size_t)m + 1) * 8 + 64));
    TSQ_HIP(h, hipMemsetAsync(mb->okoff.p, 0, ((size_t)m + 1) * 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(mb->ovoff.p, 0, ((size_t)m + 1) * 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(src.p, 0xff, (size_t)m * 4, ctx->stream));  // (-1: no entry; k_mb_copy skips it)
    a.src = src.as<int32_t>();
    a.ops = mb->oops.as<uint8_t>();
    a.okoff = mb->okoff.as<int64_t>();
    a.ovoff = mb->ovoff.as<int64_t>();
    if (n > 0) hipLaunchKernelGGL(k_mb_place, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.okoff, m, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.ovoff, m, scan_tmp));
    int64_t by[2] = {0, 0};
    TSQ_HIP(h, hipMemcpyAsync(&by[0], a.okoff + m, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&by[1], a.ovoff + m, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_TRY(mb_ctl_read(mb, &ctl));
    if (by[0] < 0 || by[0] > mb->key_used || by[1] < 0 || by[1] > mb->val_used || (int64_t)(ctl.puts + ctl.dels + ctl.locks) != m ||
        (int64_t)ctl.size != by[0] + by[1])
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the byte counts of the transaction buffer are out of range");
    int64_t primary = -1;
    if (m > 0) {
        primary = ctl.first_put != TSQ_MB_NONE ? (int64_t)ctl.first_put : (int64_t)ctl.lock_primary;
        if (primary < 0 || primary >= m) return tsq_fail(h, TSQ_ERR_HIP, "internal: the primary of the transaction buffer is out of range");
    }
    if (mb->cfg.total_size_limit > 0 && (int64_t)ctl.size > mb->cfg.total_size_limit) {
        TSQ_HIP(h, hipEventRecord(mb->ev[1], ctx->stream));
        return tsq_fail(h, TSQ_ERR_INVALID, "membuf: transaction too large");
    }
    TSQ_TRY(mb->okeys.reserve(ctx, h, (size_t)by[0] + 64));
    TSQ_TRY(mb->ovals.reserve(ctx, h, (size_t)by[1] + 64));
    MbCopyArgs c;
    memset(&c, 0, sizeof c);
    c.src = a.src, c.m = m, c.n = n;
    c.wave_copy = tsq_knob(ctx, TSQ_KNOB_ROWENC_WAVE_COPY, TSQ_MB_DEFAULT_WAVE_COPY);
    if (m > 0) {
        c.sbytes = a.keys, c.sbeg = a.kbeg, c.dst = mb->okeys.as<uint8_t>(), c.doff = a.okoff, c.src_bytes = mb->key_used, c.dst_bytes = by[0];
        hipLaunchKernelGGL(k_mb_copy, dim3(tsq_grid_for(ctx, m, 256)), dim3(256), 0, ctx->stream, c);
        if (by[1] > 0) {
            c.sbytes = mb->vals.as<uint8_t>(), c.sbeg = mb->vbeg.as<int64_t>(), c.dst = mb->ovals.as<uint8_t>(), c.doff = a.ovoff, c.src_bytes = mb->val_used,
            c.dst_bytes = by[1];
            hipLaunchKernelGGL(k_mb_copy, dim3(tsq_grid_for(ctx, m, 256)), dim3(256), 0, ctx->stream, c);
        }
    }
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(mb->ev[1], ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (hipEventElapsedTime(&ms, mb->ev[0], mb->ev[1]) == hipSuccess) kernel_ms += ms;
    mb->m = m;
    mb->okey_bytes = by[0];
    mb->oval_bytes = by[1];
    mb->finished = true;
    mb->finishes++;
    result->n_entries = m;
    result->puts = (int64_t)ctl.puts;
    result->dels = (int64_t)ctl.dels;
    result->locks = (int64_t)ctl.locks;
    result->size = (int64_t)ctl.size;
    result->primary_index = primary;
    result->sort_passes = passes;
    result->kernel_ms = kernel_ms;
    return TSQ_OK;
}
}  // namespace

TSQ_API tsq_status tsq_membuf_create(tsq_ctx* ctx, const tsq_membuf_cfg* cfg, tsq_membuf** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !out) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_membuf_create: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    std::unique_ptr<tsq_membuf> mb(new tsq_membuf());
    mb->hdr.magic = TSQ_MAGIC_MEMBUF;
    mb->ctx = ctx;
    memset(&mb->cfg, 0, sizeof mb->cfg);
    if (cfg) mb->cfg = *cfg;
    if (mb->cfg.entry_size_limit < 0 || mb->cfg.total_size_limit < 0) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_membuf_create: negative limit");
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    for (int i = 0; i < 2; i++)
        if (mb->ev[i].create() != hipSuccess) return tsq_fail(ch, TSQ_ERR_HIP, "hipEventCreate");
    *out = mb.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_membuf_push(tsq_membuf* mb, int32_t kind, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n,
                                   const uint8_t* values, const int64_t* value_offsets, int64_t value_bytes, uint32_t data_flags, int64_t* error_row) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &mb->hdr;
    if (error_row) *error_row = -1;
    if (kind != TSQ_MEMBUF_SET && kind != TSQ_MEMBUF_DELETE && kind != TSQ_MEMBUF_LOCK) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: a kind other than Set, Delete or Lock");
    const bool set = kind == TSQ_MEMBUF_SET;
    if (!set) value_bytes = 0;
    if (n < 0 || key_bytes < 0 || value_bytes < 0) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: negative count");
    if (n == 0) return TSQ_OK;
    if ((key_bytes > 0 && !keys) || (set && !value_offsets) || (value_bytes > 0 && !values)) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    if (!key_offsets && key_bytes % n != 0) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: keys of a fixed length need key_bytes to be a multiple of n");
    if (n >= (1LL << 31) || mb->n + n >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "membuf: 2^31 entries or more");
    tsq_ctx* ctx = mb->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool dev = data_flags & TSQ_COL_DEVICE;
    DevBuf tko, tvo;
    StreamDrain drain(ctx->stream);
    const size_t total = (size_t)(mb->n + n), have = (size_t)mb->n;
    TSQ_TRY(mb->keys.reserve(ctx, h, (size_t)(mb->key_used + key_bytes) + 64, true, (size_t)mb->key_used));
    TSQ_TRY(mb->vals.reserve(ctx, h, (size_t)(mb->val_used + value_bytes) + 64, true, (size_t)mb->val_used));
    for (DevBuf* b : {&mb->kbeg, &mb->klen, &mb->vbeg, &mb->vlen}) TSQ_TRY(b->reserve(ctx, h, total * 8 + 64, true, have * 8));
    TSQ_TRY(mb->kind.reserve(ctx, h, total + 64, true, have));
    TSQ_TRY(mb_copy_in(ctx, h, mb->keys.as<uint8_t>() + mb->key_used, keys, (size_t)key_bytes, dev));
    TSQ_TRY(mb_copy_in(ctx, h, mb->vals.as<uint8_t>() + mb->val_used, values, (size_t)value_bytes, dev));
    const void* d_koff = nullptr;
    const void* d_voff = nullptr;
    TSQ_TRY(mb_dev_array(ctx, h, tko, key_offsets, ((size_t)n + 1) * 8, dev, &d_koff));
    TSQ_TRY(mb_dev_array(ctx, h, tvo, set ? value_offsets : nullptr, ((size_t)n + 1) * 8, dev, &d_voff));
    MbCtl ctl;
    TSQ_TRY(mb_ctl_reset(mb, &ctl));
    MbPushArgs a;
    memset(&a, 0, sizeof a);
    a.p.koff = (const int64_t*)d_koff;
    a.p.fixed_len = key_offsets ? 0 : key_bytes / n;
    a.p.key_bytes = key_bytes;
    a.p.voff = (const int64_t*)d_voff;
    a.p.value_bytes = value_bytes;
    a.p.n = n;
    a.p.kind = kind;
    a.p.entry_limit = mb->cfg.entry_size_limit;
    a.base = mb->n, a.kbase = mb->key_used, a.vbase = mb->val_used;
    a.kbeg = mb->kbeg.as<int64_t>(), a.klen = mb->klen.as<int64_t>(), a.vbeg = mb->vbeg.as<int64_t>(), a.vlen = mb->vlen.as<int64_t>();
    a.kind = mb->kind.as<uint8_t>();
    a.ctl = mb->ctl.as<MbCtl>();
    hipLaunchKernelGGL(k_mb_push, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(mb_ctl_read(mb, &ctl));
    if (ctl.err) {  // the push adds nothing: the counts stay, what was written behind them is overwritten by the next push
        if (error_row) *error_row = ctl.first_error < (unsigned long long)n ? (int64_t)ctl.first_error : -1;
        return tsq_fail(h, TSQ_ERR_INVALID, mb_push_message(ctl.err));
    }
    mb->n += n;
    mb->key_used += key_bytes;
    mb->val_used += value_bytes;
    mb->finished = false;
    mb->forget_reads();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_membuf_finish(tsq_membuf* mb, tsq_membuf_result* result) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    if (!result) return tsq_fail(&mb->hdr, TSQ_ERR_INVALID, "tsq_membuf_finish: NULL argument");
    memset(result, 0, sizeof *result);
    result->primary_index = -1;
    return mb_finish(mb, result);
}

TSQ_API tsq_status tsq_membuf_request(tsq_membuf* mb, tsq_mvcc_write_req* req) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    if (!req) return tsq_fail(&mb->hdr, TSQ_ERR_INVALID, "tsq_membuf_request: NULL argument");
    if (!mb->finished) return tsq_fail(&mb->hdr, TSQ_ERR_INVALID, "membuf: not finished");
    memset(req, 0, sizeof *req);
    req->keys = mb->okeys.as<uint8_t>();
    req->key_offsets = mb->okoff.as<int64_t>();
    req->key_bytes = mb->okey_bytes;
    req->n_keys = mb->m;
    req->ops = mb->oops.as<uint8_t>();
    req->values = mb->ovals.as<uint8_t>();
    req->value_offsets = mb->ovoff.as<int64_t>();
    req->value_bytes = mb->oval_bytes;
    req->flags = TSQ_COL_DEVICE;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_membuf_get(tsq_membuf* mb, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n, uint32_t data_flags,
                                  int64_t* entry_out) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(mb, TSQ_MAGIC_MEMBUF));
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &mb->hdr;
    if (!mb->finished) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: not finished");
    if (n < 0 || key_bytes < 0) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: negative count");
    if (n == 0) return TSQ_OK;
    if (!entry_out || (key_bytes > 0 && !keys)) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: NULL array");
    if (!key_offsets && key_bytes % n != 0) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: keys of a fixed length need key_bytes to be a multiple of n");
    tsq_ctx* ctx = mb->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool dev = data_flags & TSQ_COL_DEVICE;
    DevBuf tk, tko, out;
    StreamDrain drain(ctx->stream);
    const void* d_keys = nullptr;
    const void* d_koff = nullptr;
    TSQ_TRY(mb_dev_array(ctx, h, tk, keys, (size_t)key_bytes, dev, &d_keys));
    TSQ_TRY(mb_dev_array(ctx, h, tko, key_offsets, ((size_t)n + 1) * 8, dev, &d_koff));
    TSQ_TRY(out.reserve(ctx, h, (size_t)n * 8 + 64));
    MbCtl ctl;
    TSQ_TRY(mb_ctl_reset(mb, &ctl));
    MbGetArgs g;
    memset(&g, 0, sizeof g);
    g.okeys = mb->okeys.as<uint8_t>(), g.okoff = mb->okoff.as<int64_t>(), g.oops = mb->oops.as<uint8_t>(), g.m = mb->m;
    g.pkeys = (const uint8_t*)d_keys, g.pkoff = (const int64_t*)d_koff, g.fixed_len = key_offsets ? 0 : key_bytes / n, g.pkey_bytes = key_bytes, g.n = n;
    g.out = out.as<int64_t>();
    g.ctl = mb->ctl.as<MbCtl>();
    hipLaunchKernelGGL(k_mb_get, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, g);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipMemcpyAsync(entry_out, out.p, (size_t)n * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_TRY(mb_ctl_read(mb, &ctl));
    if (ctl.err) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: offsets decrease or leave their buffer");
    return TSQ_OK;
}

TSQ_API void tsq_membuf_destroy(tsq_membuf* mb) {
    if (!mb || mb->hdr.magic != TSQ_MAGIC_MEMBUF) return;
    {
        tsq_ctx_lock _api_lock(mb->ctx);
        (void)hipSetDevice(mb->ctx->device);
        (void)hipStreamSynchronize(mb->ctx->stream);
        mb->hdr.magic = 0;
    }
    delete mb;
}
