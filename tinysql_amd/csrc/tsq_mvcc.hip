// tsq_mvcc.hip — the MVCC snapshot read on the GPU (gfx950): a versioned store in HBM and the reference's Scan / ReverseScan / Get
// over key ranges at a startTS (store/mockstore/mocktikv/mvcc_leveldb.go:261-430, mvcc.go:187-227; include/tsq.h "MVCC snapshot
// read").  The per-key code is tsq_mvcc_dp.h.
//
// tsq_mvcc_create (once per store):
//   K21a k_mv_entries   : one lane per version — its offset pairs, then its key against the version before it (order, head flag),
//                         commitTS order inside a key, type, the empty put
//   K21b k_mv_lockcheck : one lane per lock — offsets, order, op
//        (the host reads the error word; phase two runs on a store that passed)
//        tsq_launch_scan64: head flags -> key ordinals, K
//   K21c k_mv_ordinals  : the ordinal of every version, the K + 1 segment starts
//   K21d k_mv_lockfind  : one lane per lock — its lower bound among the K keys, whether it is one of them; orphans are counted per bound
//        tsq_launch_scan64 x 2: orphans before every key, the rank of every orphan
//   K21e k_mv_universe_keys / K21f k_mv_universe_locks: the key universe — key bytes, first version, version count, lock or -1
// tsq_mvcc_scan (per read):
//   K21g k_mv_bounds    : one lane per range — two bound searches over the universe (or one and an equality test for a point)
//        tsq_launch_scan64: interval lengths -> the position space; the host reads its size
//   K21h k_mv_resolve   : one lane per position — range of the position, key, lock check, chain walk; chains of the threshold length or
//                         more are taken by the whole wave in 64-version steps; per-wave pair counts, atomicMin of the first locked position
//        k_compact_scan (tsq_compact.h): the counts -> exclusive bases + the total
//   K21i k_mv_scatter   : ballot + popcount prefix -> the chosen entries and their positions, in scan order, up to the limit
//   K21j k_mv_decide    : one lane — pairs before the first locked position against the limit: success or ErrLocked, the lock's fields
//   K21k k_mv_lens      : key and value length of every returned pair; tsq_launch_scan64 x 2 -> the output offsets and byte totals
//   K21l k_mv_range_counts: one lane per range — its pairs after the limit, by two searches over the returned positions
// tsq_mvcc_fetch: K18f k_rg_copy (tsq_lookup.hip) twice — the keys, then the values; long cells are copied by a wave
#include "tsq_compact.h"
#include "tsq_lookup_dp.h"
#include "tsq_mvcc_store.h"

#define TSQ_MV_DEFAULT_WAVE_CHAIN 64  // TSQ_KNOB_MVCC_WAVE_CHAIN: 16 .. 4096 measure equal (profiles/mvcc_scan_ab.txt); one wave step
#define TSQ_MV_E_RANGE_OFFSETS 1u

struct MvCreateArgs {
    const uint8_t* keys;  // the store's keys, then the locks' keys
    const int64_t* koff;
    int64_t key_bytes;
    const uint64_t* cts;
    const uint8_t* types;
    const int64_t* voff;
    int64_t value_bytes;
    int64_t n;
    const int64_t* lkoff;
    int64_t lkey_bytes;
    const uint8_t* lops;
    const int64_t* lpoff;
    int64_t lprim_bytes;
    int64_t n_locks;
    unsigned int* err;
    uint8_t* head;   // [n]
    int64_t* scanv;  // [n + 1]: head flags, then (scan) the heads before every version; scanv[n] = K
    int32_t* ord;    // [n]
    int32_t* seg;    // [n + 1]
    int32_t* llb;    // [n_locks]: the lock's lower bound among the K keys
    uint8_t* leq;    // [n_locks]: it is that key
    int64_t* add;    // [n + 2]: orphans per bound, then (scan) orphans before every bound
    int64_t* oscan;  // [n_locks + 1]: orphan flags, then ranks
    int64_t* ubeg;   // the universe, [n + n_locks]
    int32_t* ulen;
    int32_t* useg;
    int32_t* ucnt;
    int32_t* ulock;
};

__global__ void __launch_bounds__(256) k_mv_entries(MvCreateArgs a) {
    unsigned int e = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        bool head = true;
        e |= tsq_mv_entry_check(a.keys, a.koff, a.key_bytes, a.cts, a.types, a.voff, a.value_bytes, i, &head);
        a.head[i] = head ? 1 : 0;
        a.scanv[i] = head ? 1 : 0;
    }
    if (e) atomicOr(a.err, e);
}
__global__ void __launch_bounds__(256) k_mv_lockcheck(MvCreateArgs a) {
    unsigned int e = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n_locks; j += (int64_t)gridDim.x * blockDim.x)
        e |= tsq_mv_lock_entry_check(a.keys + a.key_bytes, a.lkoff, a.lkey_bytes, a.lops, a.lpoff, a.lprim_bytes, j);
    if (e) atomicOr(a.err, e);
}
__global__ void __launch_bounds__(256) k_mv_ordinals(MvCreateArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.n; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = a.scanv[i] + a.head[i] - 1;  // (entry 0 is a head: o >= 0; o < K <= n)
        a.ord[i] = (int32_t)o;
        if (a.head[i]) a.seg[o] = (int32_t)i;
        if (i == a.n - 1) a.seg[o + 1] = (int32_t)a.n;
    }
}
__global__ void __launch_bounds__(256) k_mv_lockfind(MvCreateArgs a) {
    const int64_t K = a.scanv[a.n];
    const uint8_t* lkeys = a.keys + a.key_bytes;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n_locks; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t b = a.lkoff[j], len = a.lkoff[j + 1] - b;
        const int64_t lb = tsq_mv_lower_heads(a.keys, a.koff, a.seg, K, lkeys + b, len);
        bool eq = false;
        if (lb < K) {
            const int64_t e = a.seg[lb], kb = a.koff[e];
            eq = tsq_dc_bytes_equal(a.keys + kb, a.koff[e + 1] - kb, lkeys + b, len);
        }
        a.llb[j] = (int32_t)lb;
        a.leq[j] = eq ? 1 : 0;
        a.oscan[j] = eq ? 0 : 1;
        if (!eq) atomicAdd((unsigned long long*)&a.add[lb], 1ull);  // (lb <= K <= n: add has n + 2 entries)
    }
}
// key k of the K keys with versions sits behind the orphans whose bound is <= k: add[k + 1] after the exclusive scan
__global__ void __launch_bounds__(256) k_mv_universe_keys(MvCreateArgs a) {
    const int64_t K = a.scanv[a.n];
    for (int64_t k = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; k < K; k += (int64_t)gridDim.x * blockDim.x) {
        const int64_t u = k + a.add[k + 1];
        const int64_t e = a.seg[k];
        a.ubeg[u] = a.koff[e];
        a.ulen[u] = (int32_t)(a.koff[e + 1] - a.koff[e]);
        a.useg[u] = (int32_t)e;
        a.ucnt[u] = a.seg[k + 1] - (int32_t)e;
        a.ulock[u] = -1;
    }
}
// (after k_mv_universe_keys on the stream: the lock of a key with versions overwrites its -1)
__global__ void __launch_bounds__(256) k_mv_universe_locks(MvCreateArgs a) {
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.n_locks; j += (int64_t)gridDim.x * blockDim.x) {
        const int64_t lb = a.llb[j];
        if (a.leq[j]) {
            a.ulock[lb + a.add[lb + 1]] = (int32_t)j;
        } else {
            const int64_t u = lb + a.oscan[j];  // the keys before it + the orphans before it
            a.ubeg[u] = a.key_bytes + a.lkoff[j];
            a.ulen[u] = (int32_t)(a.lkoff[j + 1] - a.lkoff[j]);
            a.useg[u] = a.seg[lb];  // where its versions would go: the first entry of the next key that has some (seg[K] = n)
            a.ucnt[u] = 0;
            a.ulock[u] = (int32_t)j;
        }
    }
}

struct MvScanArgs {
    tsq_mv_store s;
    const uint64_t* l_ttl;
    const int64_t* koff;  // per entry
    const int64_t* voff;
    const uint8_t* rbytes;  // the ranges
    const int64_t* roffs;   // [2 R + 1]
    const uint32_t* rflags; // [R] or nullptr
    int64_t rbytes_n;
    int64_t R;
    int32_t* rlo;    // [R]
    int64_t* rbase;  // [R + 1]: interval lengths, then (scan) positions before every range
    int64_t P;
    uint64_t ts;
    int32_t desc;
    int64_t chain_wave;
    int64_t rows_per_wave;  // a multiple of 64
    int32_t* chosen;        // [P]: the entry whose pair the position yields, or -1
    unsigned long long* block_base;
    MvCtl* ctl;
    int64_t M;            // min(P, limit): the most pairs the call can return
    int64_t limit;        // INT64_MAX: none
    int64_t* sel;         // [M]
    int64_t* selpos;      // [M]
    int64_t* klens;       // [M + 1]
    int64_t* vlens;       // [M + 1]
    int64_t* rcounts;     // [R]
};

__global__ void __launch_bounds__(256) k_mv_bounds(MvScanArgs a) {
    unsigned int e = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o0 = a.roffs[2 * r], o1 = a.roffs[2 * r + 1], o2 = a.roffs[2 * r + 2];
        int64_t lo = 0, cnt = 0;
        if (o0 < 0 || o1 < o0 || o2 < o1 || o2 > a.rbytes_n) e |= TSQ_MV_E_RANGE_OFFSETS;
        else tsq_mv_bounds(a.s.k, a.rbytes + o0, o1 - o0, a.rbytes + o1, o2 - o1, a.rflags ? a.rflags[r] : 0u, &lo, &cnt);
        a.rlo[r] = (int32_t)lo;
        a.rbase[r] = cnt;
    }
    if (e) atomicOr(&a.ctl->err, e);
}

__global__ void __launch_bounds__(256) k_mv_resolve(MvScanArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = w * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.P ? hi : a.P;
    unsigned int c = 0;
    unsigned long long first = ~0ull;
    int64_t walked = 0;
    for (int64_t p0 = lo; p0 < hi; p0 += 64) {  // (wave uniform trip count: lo and hi are)
        const int64_t p = p0 + lane;
        const bool in = p < hi;
        int64_t res = -1, s = 0, e = 0;
        uint64_t ts = a.ts;
        bool locked = false, by_wave = false;
        if (in) {
            const int64_t r = a.R == 1 ? 0 : tsq_mv_range_of(a.rbase, a.R, p);
            const int64_t rb = a.rbase[r];
            const int64_t u = tsq_mv_key_at(a.rlo[r], a.rbase[r + 1] - rb, p - rb, a.desc);
            locked = tsq_mv_key_lock(a.s, u, &ts) != 0;
            if (!locked) {
                s = a.s.seg[u];
                e = s + a.s.cnt[u];
                by_wave = a.chain_wave > 0 && e - s >= a.chain_wave;
                if (!by_wave) res = tsq_mv_walk(a.s.cts, a.s.types, s, e, ts, &walked);
            }
        }
        unsigned long long todo = __ballot(by_wave);
        while (todo) {  // (wave uniform)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t we = (int64_t)__shfl((unsigned long long)e, src, 64);
            const uint64_t wts = __shfl((unsigned long long)ts, src, 64);
            int64_t steps = 0;
            int64_t i0 = tsq_mv_first_le(a.s.cts, (int64_t)__shfl((unsigned long long)s, src, 64), we, wts, &steps);  // (every lane the same search)
            int64_t found = -1;
            while (i0 < we) {  // (wave uniform)
                const unsigned long long bal = __ballot(tsq_mv_decides(a.s.types, i0 + lane, we));
                steps += we - i0 < 64 ? we - i0 : 64;
                if (bal) {
                    found = i0 + (__ffsll((long long)bal) - 1);
                    break;
                }
                i0 += 64;
            }
            if (lane == src) {
                res = found >= 0 ? tsq_mv_verdict(a.s.types, found) : -1;
                walked += steps;
            }
        }
        if (in) {
            a.chosen[p] = (int32_t)res;
            if (locked && (unsigned long long)p < first) first = (unsigned long long)p;
        }
        c += res >= 0 ? 1u : 0u;
    }
    unsigned long long wk = (unsigned long long)walked;
    for (int o = 32; o > 0; o >>= 1) {
        c += __shfl_xor(c, o, 64);
        wk += __shfl_xor(wk, o, 64);
        const unsigned long long f = __shfl_xor(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        a.block_base[w] = c;
        if (wk) atomicAdd(&a.ctl->walked, wk);
        if (first != ~0ull) atomicMin(&a.ctl->first_locked, first);
    }
}
__global__ void __launch_bounds__(256) k_mv_scatter(MvScanArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t w = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);
    const int64_t lo = w * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.P ? hi : a.P;
    unsigned long long cur = a.block_base[w];
    const unsigned long long lt = (1ull << lane) - 1ull;
    for (int64_t p0 = lo; p0 < hi; p0 += 64) {  // (wave uniform)
        const int64_t p = p0 + lane;
        const int32_t ch = p < hi ? a.chosen[p] : -1;
        const bool hit = ch >= 0;
        const unsigned long long bal = __ballot(hit);
        const unsigned long long at = cur + (unsigned long long)__popcll(bal & lt);
        if (hit && at < (unsigned long long)a.M) {
            a.sel[at] = ch;
            a.selpos[at] = p;
        }
        cur += (unsigned long long)__popcll(bal);
    }
}
__global__ void __launch_bounds__(64) k_mv_decide(MvScanArgs a) {
    if (threadIdx.x != 0) return;
    MvCtl* c = a.ctl;
    const int64_t T = (int64_t)c->total;
    const int64_t Tm = T < a.M ? T : a.M;
    const unsigned long long L = c->first_locked;
    const bool any = L < (unsigned long long)a.P;
    const int64_t before = any ? tsq_mv_lower_i64(a.selpos, Tm, (int64_t)L) : Tm;
    if (any && before < a.limit) {
        const int64_t r = tsq_mv_range_of(a.rbase, a.R, (int64_t)L);
        const int64_t rb = a.rbase[r];
        const int64_t u = tsq_mv_key_at(a.rlo[r], a.rbase[r + 1] - rb, (int64_t)L - rb, a.desc);
        const int32_t j = a.s.lock[u];  // (>= 0: the position was locked)
        c->locked = 1;
        c->n_pairs = before;
        c->n_fetch = 0;
        c->lock_j = j;
        c->key_beg = a.s.k.beg[u];
        c->key_len = a.s.k.len[u];
        c->prim_beg = a.s.l_poff[j];
        c->prim_len = a.s.l_poff[j + 1] - a.s.l_poff[j];
        c->l_start = a.s.l_start[j];
        c->l_ttl = a.l_ttl[j];
        c->l_op = a.s.l_op[j];
    } else {
        c->locked = 0;
        c->n_pairs = Tm;
        c->n_fetch = Tm;
    }
}
__global__ void __launch_bounds__(256) k_mv_lens(MvScanArgs a) {
    const int64_t n = a.ctl->n_fetch;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.M; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t kl = 0, vl = 0;
        if (i < n) {
            const int64_t e = a.sel[i];
            kl = a.koff[e + 1] - a.koff[e];
            vl = a.voff[e + 1] - a.voff[e];
        }
        a.klens[i] = kl;
        a.vlens[i] = vl;
    }
}
__global__ void __launch_bounds__(256) k_mv_range_counts(MvScanArgs a) {
    const int64_t n = a.ctl->n_fetch;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x)
        a.rcounts[r] = tsq_mv_lower_i64(a.selpos, n, a.rbase[r + 1]) - tsq_mv_lower_i64(a.selpos, n, a.rbase[r]);
}

// ====================================================================== host side
// (the handle: tsq_mvcc_store.h)
namespace {
tsq_status mv_cancelled(tsq_mvcc* m) {
    if (m->cancelled.load()) return tsq_fail(&m->hdr, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    return TSQ_OK;
}
// several checks may fail at once: the message is the first of this order (offsets, empty key, enum ranges, then the orders)
const char* mv_create_message(unsigned int e) {
    if (e & TSQ_MV_E_OFFSETS) return "mvcc store: offsets decrease or leave their buffer";
    if (e & TSQ_MV_E_EMPTY_KEY) return "mvcc store: empty key";
    if (e & TSQ_MV_E_TYPE) return "mvcc store: value type or lock op out of range";
    if (e & TSQ_MV_E_KEY_ORDER) return "mvcc store: keys not ascending";
    if (e & TSQ_MV_E_VERSION_ORDER) return "mvcc store: versions of a key not descending in commitTS";
    if (e & TSQ_MV_E_EMPTY_PUT) return "mvcc store: a put with an empty value";
    if (e & TSQ_MV_E_LOCK_ORDER) return "mvcc store: lock keys not ascending";
    return "mvcc store: two locks on one key";
}
// the caller's arrays into the handle's own buffers
tsq_status mv_copy(tsq_mvcc* m, tsq_handle_hdr* ch, const tsq_mvcc_data* d) {
    tsq_ctx* ctx = m->ctx;
    const bool dev = d->data_flags & TSQ_COL_DEVICE;
    const int64_t n = d->n, nl = d->n_locks;
    const size_t kb = (size_t)d->key_bytes, lkb = (size_t)d->lock_key_bytes;
    static const int64_t zero_off = 0;  // an empty list may come without its offsets
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->keys, d->keys, kb, dev, 0, kb + lkb));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->keys, d->lock_keys, lkb, dev, kb, kb + lkb));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->koff, n ? (const void*)d->key_offsets : &zero_off, ((size_t)n + 1) * 8, n ? dev : false));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->cts, d->commit_ts, (size_t)n * 8, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->types, d->types, (size_t)n, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->vals, d->values, (size_t)d->value_bytes, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->voff, n ? (const void*)d->value_offsets : &zero_off, ((size_t)n + 1) * 8, n ? dev : false));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lkoff, nl ? (const void*)d->lock_key_offsets : &zero_off, ((size_t)nl + 1) * 8, nl ? dev : false));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lstart, d->lock_start_ts, (size_t)nl * 8, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lttl, d->lock_ttl, (size_t)nl * 8, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lops, d->lock_ops, (size_t)nl, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lprim, d->lock_primaries, (size_t)d->lock_primary_bytes, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lpoff, nl ? (const void*)d->lock_primary_offsets : &zero_off, ((size_t)nl + 1) * 8, nl ? dev : false));
    return TSQ_OK;
}
}  // namespace

tsq_status tsq_mv_copy_in(tsq_ctx* ctx, tsq_handle_hdr* h, DevBuf& b, const void* src, size_t bytes, bool dev, size_t at, size_t room) {
    TSQ_TRY(b.reserve(ctx, h, std::max(bytes + at, room) + 64));
    if (bytes) TSQ_HIP(h, hipMemcpyAsync((char*)b.p + at, src, bytes, dev ? hipMemcpyDeviceToDevice : hipMemcpyHostToDevice, ctx->stream));
    return TSQ_OK;
}

tsq_status tsq_mv_index(tsq_mvcc* m, tsq_handle_hdr* ch, bool internal) {
    tsq_ctx* ctx = m->ctx;
    const int64_t n = m->n, nl = m->n_locks;
    TSQ_TRY(m->head.reserve(ctx, ch, (size_t)n + 64));
    TSQ_TRY(m->ord.reserve(ctx, ch, (size_t)n * 4 + 64));
    TSQ_TRY(m->seg.reserve(ctx, ch, ((size_t)n + 1) * 4 + 64));
    TSQ_TRY(m->ctl.reserve(ctx, ch, sizeof(MvCtl) + 64));
    const size_t un = (size_t)n + (size_t)nl;
    TSQ_TRY(m->ubeg.reserve(ctx, ch, un * 8 + 64));
    for (DevBuf* b : {&m->ulen, &m->useg, &m->ucnt, &m->ulock}) TSQ_TRY(b->reserve(ctx, ch, un * 4 + 64));
    DevBuf scanv, llb, leq, add, oscan;
    StreamDrain drain(ctx->stream);  // every exit below waits for the kernels that use the five buffers
    TSQ_TRY(scanv.reserve(ctx, ch, ((size_t)n + 1) * 8 + 64));
    TSQ_TRY(llb.reserve(ctx, ch, (size_t)nl * 4 + 64));
    TSQ_TRY(leq.reserve(ctx, ch, (size_t)nl + 64));
    TSQ_TRY(add.reserve(ctx, ch, ((size_t)n + 3) * 8 + 64));
    TSQ_TRY(oscan.reserve(ctx, ch, ((size_t)nl + 1) * 8 + 64));
    MvCreateArgs a;
    memset(&a, 0, sizeof a);
    a.keys = m->keys.as<uint8_t>();
    a.koff = m->koff.as<int64_t>();
    a.key_bytes = m->key_bytes;
    a.cts = m->cts.as<uint64_t>();
    a.types = m->types.as<uint8_t>();
    a.voff = m->voff.as<int64_t>();
    a.value_bytes = m->value_bytes;
    a.n = n;
    a.lkoff = m->lkoff.as<int64_t>();
    a.lkey_bytes = m->lkey_bytes;
    a.lops = m->lops.as<uint8_t>();
    a.lpoff = m->lpoff.as<int64_t>();
    a.lprim_bytes = m->lprim_bytes;
    a.n_locks = nl;
    a.err = &m->ctl.as<MvCtl>()->err;
    a.head = m->head.as<uint8_t>();
    a.scanv = scanv.as<int64_t>();
    a.ord = m->ord.as<int32_t>();
    a.seg = m->seg.as<int32_t>();
    a.llb = llb.as<int32_t>();
    a.leq = leq.as<uint8_t>();
    a.add = add.as<int64_t>();
    a.oscan = oscan.as<int64_t>();
    a.ubeg = m->ubeg.as<int64_t>();
    a.ulen = m->ulen.as<int32_t>();
    a.useg = m->useg.as<int32_t>();
    a.ucnt = m->ucnt.as<int32_t>();
    a.ulock = m->ulock.as<int32_t>();
    auto hip_fail = [&](hipError_t e) { return tsq_fail(ch, TSQ_ERR_HIP, std::string("tsq_mvcc_create: ") + hipGetErrorString(e)); };
    hipError_t e = hipMemsetAsync(m->ctl.p, 0, sizeof(MvCtl), ctx->stream);
    if (e == hipSuccess) e = hipMemsetAsync(a.seg, 0, 8, ctx->stream);  // (an empty store: seg[0] = 0)
    if (e == hipSuccess && n > 0) hipLaunchKernelGGL(k_mv_entries, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
    if (e == hipSuccess && nl > 0) hipLaunchKernelGGL(k_mv_lockcheck, dim3(tsq_grid_for(ctx, nl, 256)), dim3(256), 0, ctx->stream, a);
    if (e == hipSuccess) e = hipGetLastError();
    unsigned int err = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&err, a.err, 4, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    if (err && internal) return tsq_fail(ch, TSQ_ERR_HIP, std::string("internal: the next store fails the create checks: ") + mv_create_message(err));
    if (err) return tsq_fail(ch, TSQ_ERR_INVALID, mv_create_message(err));
    // phase two: the store passed, every offset and order below holds
    TSQ_TRY(tsq_launch_scan64(ctx, ch, a.scanv, n, m->scan_tmp));
    e = hipMemsetAsync(a.add, 0, ((size_t)n + 3) * 8, ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    if (n > 0) hipLaunchKernelGGL(k_mv_ordinals, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
    if (nl > 0) hipLaunchKernelGGL(k_mv_lockfind, dim3(tsq_grid_for(ctx, nl, 256)), dim3(256), 0, ctx->stream, a);
    e = hipGetLastError();
    if (e != hipSuccess) return hip_fail(e);
    TSQ_TRY(tsq_launch_scan64(ctx, ch, a.add, n + 1, m->scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, ch, a.oscan, nl, m->scan_tmp));
    if (n > 0) hipLaunchKernelGGL(k_mv_universe_keys, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
    if (nl > 0) hipLaunchKernelGGL(k_mv_universe_locks, dim3(tsq_grid_for(ctx, nl, 256)), dim3(256), 0, ctx->stream, a);
    e = hipGetLastError();
    int64_t K = 0, orphans = 0;
    if (e == hipSuccess) e = hipMemcpyAsync(&K, a.scanv + n, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipMemcpyAsync(&orphans, a.oscan + nl, 8, hipMemcpyDeviceToHost, ctx->stream);
    if (e == hipSuccess) e = hipStreamSynchronize(ctx->stream);
    if (e != hipSuccess) return hip_fail(e);
    if (K < 0 || K > n || orphans < 0 || orphans > nl) return tsq_fail(ch, TSQ_ERR_HIP, "internal: the key count of the mvcc store is out of range");
    m->K = K;
    m->U = K + orphans;
    return TSQ_OK;
}
void tsq_mv_store_view(const tsq_mvcc* m, tsq_mv_store* s) {
    s->k.bytes = m->keys.as<uint8_t>();
    s->k.beg = m->ubeg.as<int64_t>();
    s->k.len = m->ulen.as<int32_t>();
    s->k.n = m->U;
    s->seg = m->useg.as<int32_t>();
    s->cnt = m->ucnt.as<int32_t>();
    s->lock = m->ulock.as<int32_t>();
    s->cts = m->cts.as<uint64_t>();
    s->types = m->types.as<uint8_t>();
    s->l_start = m->lstart.as<uint64_t>();
    s->l_op = m->lops.as<uint8_t>();
    s->l_prim = m->lprim.as<uint8_t>();
    s->l_poff = m->lpoff.as<int64_t>();
}
tsq_status tsq_mv_new(tsq_ctx* ctx, tsq_handle_hdr* ch, std::unique_ptr<tsq_mvcc>* out) {
    std::unique_ptr<tsq_mvcc> m(new tsq_mvcc());
    m->hdr.magic = TSQ_MAGIC_MVCC;
    m->ctx = ctx;
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    for (int i = 0; i < 4; i++)
        if (m->ev[i].create() != hipSuccess) return tsq_fail(ch, TSQ_ERR_HIP, "hipEventCreate");
    *out = std::move(m);
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_create(tsq_ctx* ctx, const tsq_mvcc_data* d, tsq_mvcc** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !out || !d) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_mvcc_create: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (d->n < 0 || d->n_locks < 0 || d->key_bytes < 0 || d->value_bytes < 0 || d->lock_key_bytes < 0 || d->lock_primary_bytes < 0)
        return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_mvcc_create: negative count");
    if (d->n >= (1LL << 31) || d->n_locks >= (1LL << 31) || d->n + d->n_locks >= (1LL << 31)) return tsq_fail(ch, TSQ_ERR_UNSUPPORTED, "mvcc store: 2^31 entries or more");
    if ((d->n > 0 && (!d->key_offsets || !d->commit_ts || !d->types || !d->value_offsets)) || (d->key_bytes > 0 && !d->keys) ||
        (d->value_bytes > 0 && !d->values) ||
        (d->n_locks > 0 && (!d->lock_key_offsets || !d->lock_start_ts || !d->lock_ttl || !d->lock_ops || !d->lock_primary_offsets)) ||
        (d->lock_key_bytes > 0 && !d->lock_keys) || (d->lock_primary_bytes > 0 && !d->lock_primaries))
        return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_mvcc_create: NULL array");
    std::unique_ptr<tsq_mvcc> m;
    TSQ_TRY(tsq_mv_new(ctx, ch, &m));
    m->n = d->n;
    m->n_locks = d->n_locks;
    m->key_bytes = d->key_bytes;
    m->value_bytes = d->value_bytes;
    m->lkey_bytes = d->lock_key_bytes;
    m->lprim_bytes = d->lock_primary_bytes;
    tsq_status st = mv_copy(m.get(), ch, d);
    if (st == TSQ_OK) st = tsq_mv_index(m.get(), ch, false);
    if (st != TSQ_OK) {
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return st;
    }
    *out = m.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_scan(tsq_mvcc* m, const uint8_t* range_bytes, const int64_t* range_offsets, const uint32_t* range_flags, int64_t n_ranges,
                                 uint64_t start_ts, int32_t desc, int64_t limit, tsq_mvcc_result* result, int64_t* range_counts) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (result) memset(result, 0, sizeof *result);
    m->have_last = false;
    TSQ_TRY(mv_cancelled(m));
    if (!result || n_ranges < 0 || (n_ranges > 0 && !range_offsets)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_scan: bad arguments");
    if (n_ranges >= (1LL << 30)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "mvcc scan: 2^30 ranges or more");
    const int64_t R = n_ranges;
    const int64_t rb_n = R > 0 ? range_offsets[2 * R] : 0;  // (checked against every offset on the device)
    if (rb_n < 0 || (rb_n > 0 && !range_bytes)) return tsq_fail(h, TSQ_ERR_INVALID, "mvcc scan: range offsets decrease or leave the range bytes");
    m->scans++;
    memset(&m->last, 0, sizeof m->last);
    m->last_key_bytes = m->last_value_bytes = 0;
    if (range_counts && R > 0) memset(range_counts, 0, (size_t)R * 8);
    if (R == 0 || m->U == 0 || limit == 0) {
        m->have_last = true;
        return TSQ_OK;
    }
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    MvScanArgs a;
    memset(&a, 0, sizeof a);
    tsq_mv_store_view(m, &a.s);
    a.l_ttl = m->lttl.as<uint64_t>();
    a.koff = m->koff.as<int64_t>();
    a.voff = m->voff.as<int64_t>();
    TSQ_TRY(tsq_mv_copy_in(ctx, h, m->rbytes, range_bytes, (size_t)rb_n, false));
    TSQ_TRY(tsq_mv_copy_in(ctx, h, m->roffs, range_offsets, ((size_t)2 * R + 1) * 8, false));
    if (range_flags) TSQ_TRY(tsq_mv_copy_in(ctx, h, m->rflags, range_flags, (size_t)R * 4, false));
    TSQ_TRY(m->rlo.reserve(ctx, h, (size_t)R * 4 + 64));
    TSQ_TRY(m->rbase.reserve(ctx, h, ((size_t)R + 1) * 8 + 64));
    TSQ_TRY(m->rcounts.reserve(ctx, h, (size_t)R * 8 + 64));
    a.rbytes = m->rbytes.as<uint8_t>();
    a.roffs = m->roffs.as<int64_t>();
    a.rflags = range_flags ? m->rflags.as<uint32_t>() : nullptr;
    a.rbytes_n = rb_n;
    a.R = R;
    a.rlo = m->rlo.as<int32_t>();
    a.rbase = m->rbase.as<int64_t>();
    a.rcounts = m->rcounts.as<int64_t>();
    a.ctl = m->ctl.as<MvCtl>();
    a.ts = start_ts;
    a.desc = desc ? 1 : 0;
    a.chain_wave = tsq_knob(ctx, TSQ_KNOB_MVCC_WAVE_CHAIN, TSQ_MV_DEFAULT_WAVE_CHAIN);
    a.limit = limit < 0 ? INT64_MAX : limit;
    TSQ_HIP(h, hipMemsetAsync(a.ctl, 0, sizeof(MvCtl), ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(&a.ctl->first_locked, 0xff, 8, ctx->stream));
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_mv_bounds, dim3(tsq_grid_for(ctx, R, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.rbase, R, m->scan_tmp));
    int64_t P = 0;
    unsigned int rerr = 0;
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&P, a.rbase + R, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&rerr, &a.ctl->err, 4, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, m->ev[0], m->ev[1]) == hipSuccess) m->kernel_ms += ms;
    if (rerr) return tsq_fail(h, TSQ_ERR_INVALID, "mvcc scan: range offsets decrease or leave the range bytes");
    if (P < 0 || P >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "mvcc scan: 2^31 scan positions or more");
    m->examined += P;
    result->positions = P;
    if (P == 0) {
        m->have_last = true;
        return TSQ_OK;
    }
    a.P = P;
    a.M = std::min<int64_t>(P, a.limit);
    const int grid = tsq_grid_for(ctx, P, 256);
    const int n_runs = grid * 4;
    a.rows_per_wave = (((P + n_runs - 1) / n_runs) + 63) & ~(int64_t)63;
    TSQ_TRY(m->chosen.reserve(ctx, h, (size_t)P * 4 + 64));
    TSQ_TRY(m->bbase.reserve(ctx, h, (size_t)n_runs * 8 + 64));
    TSQ_TRY(m->sel.reserve(ctx, h, (size_t)a.M * 8 + 64));
    TSQ_TRY(m->selpos.reserve(ctx, h, (size_t)a.M * 8 + 64));
    TSQ_TRY(m->klens.reserve(ctx, h, ((size_t)a.M + 1) * 8 + 64));
    TSQ_TRY(m->vlens.reserve(ctx, h, ((size_t)a.M + 1) * 8 + 64));
    a.chosen = m->chosen.as<int32_t>();
    a.block_base = m->bbase.as<unsigned long long>();
    a.sel = m->sel.as<int64_t>();
    a.selpos = m->selpos.as<int64_t>();
    a.klens = m->klens.as<int64_t>();
    a.vlens = m->vlens.as<int64_t>();
    TSQ_HIP(h, hipEventRecord(m->ev[2], ctx->stream));
    hipLaunchKernelGGL(k_mv_resolve, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, a.block_base, n_runs, &a.ctl->total);
    hipLaunchKernelGGL(k_mv_scatter, dim3(grid), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_mv_decide, dim3(1), dim3(64), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_mv_lens, dim3(tsq_grid_for(ctx, a.M, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.klens, a.M, m->scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.vlens, a.M, m->scan_tmp));
    hipLaunchKernelGGL(k_mv_range_counts, dim3(tsq_grid_for(ctx, R, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(m->ev[3], ctx->stream));
    int64_t kb = 0, vb = 0;
    TSQ_HIP(h, hipMemcpyAsync(&m->last, a.ctl, sizeof(MvCtl), hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&kb, a.klens + a.M, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&vb, a.vlens + a.M, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (range_counts) TSQ_HIP(h, hipMemcpyAsync(range_counts, a.rcounts, (size_t)R * 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (hipEventElapsedTime(&ms, m->ev[2], m->ev[3]) == hipSuccess) m->kernel_ms += ms;  // (the host's read-back between the two intervals is not device time)
    m->walked += (int64_t)m->last.walked;
    result->n_pairs = m->last.n_pairs;
    if (m->last.locked) {
        if (range_counts) memset(range_counts, 0, (size_t)R * 8);
        m->have_last = true;  // (for tsq_mvcc_locked; n_fetch = 0: nothing to fetch)
        return tsq_fail(h, TSQ_ERR_LOCKED, "mvcc scan: key is locked");
    }
    if (m->last.n_pairs < 0 || m->last.n_pairs > a.M || m->last.n_fetch != m->last.n_pairs || kb < 0 || vb < 0)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the counts of the mvcc scan are out of range");
    m->pairs += m->last.n_pairs;
    m->last_key_bytes = kb;
    m->last_value_bytes = vb;
    result->key_bytes = kb;
    result->value_bytes = vb;
    m->have_last = true;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_fetch(tsq_mvcc* m, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* values, int64_t value_cap,
                                  int64_t* value_offsets) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    TSQ_TRY(mv_cancelled(m));
    if (!m->have_last || m->last.locked) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_fetch: no successful scan to fetch");
    if (!key_offsets || !value_offsets || key_cap < 0 || value_cap < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_fetch: bad arguments");
    if (key_cap < m->last_key_bytes || value_cap < m->last_value_bytes || (m->last_key_bytes > 0 && !keys) || (m->last_value_bytes > 0 && !values))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_fetch: output buffer too small");
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const int64_t n = m->last.n_fetch;
    if (n == 0) {
        TSQ_HIP(h, hipMemsetAsync(key_offsets, 0, 8, ctx->stream));
        TSQ_HIP(h, hipMemsetAsync(value_offsets, 0, 8, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        return TSQ_OK;
    }
    RgArgs g;
    memset(&g, 0, sizeof g);
    g.rows = m->sel.as<int64_t>();
    g.n = n;
    g.n_src_rows = m->n;
    g.wave_copy = tsq_knob(ctx, TSQ_KNOB_GATHER_WAVE_COPY, 64);
    g.values = m->keys.as<uint8_t>();
    g.n_bytes = m->key_bytes;
    g.offsets = m->koff.as<int64_t>();
    g.lens = m->klens.as<int64_t>();
    g.out = keys;
    g.out_offsets = key_offsets;
    TSQ_TRY(tsq_launch_rg_copy(ctx, h, g));
    g.values = m->vals.as<uint8_t>();
    g.n_bytes = m->value_bytes;
    g.offsets = m->voff.as<int64_t>();
    g.lens = m->vlens.as<int64_t>();
    g.out = values;
    g.out_offsets = value_offsets;
    TSQ_TRY(tsq_launch_rg_copy(ctx, h, g));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_locked(tsq_mvcc* m, uint8_t* key, int64_t key_cap, int64_t* key_len, uint8_t* primary, int64_t primary_cap,
                                   int64_t* primary_len, uint64_t* start_ts, uint64_t* ttl, int32_t* op) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    TSQ_TRY(mv_cancelled(m));
    if (!m->have_last || !m->last.locked) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_locked: the last scan met no lock");
    const MvCtl& c = m->last;
    if (c.key_len < 0 || c.key_beg < 0 || c.key_beg + c.key_len > m->key_bytes + m->lkey_bytes || c.prim_len < 0 || c.prim_beg < 0 ||
        c.prim_beg + c.prim_len > m->lprim_bytes)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the lock of the mvcc scan is out of range");
    if (key_len) *key_len = c.key_len;
    if (primary_len) *primary_len = c.prim_len;
    if (start_ts) *start_ts = c.l_start;
    if (ttl) *ttl = c.l_ttl;
    if (op) *op = (int32_t)c.l_op;
    if (key_cap < c.key_len || primary_cap < c.prim_len || (c.key_len > 0 && !key) || (c.prim_len > 0 && !primary))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_locked: buffer too small (the lengths are filled in)");
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    if (c.key_len) TSQ_HIP(h, hipMemcpyAsync(key, m->keys.as<uint8_t>() + c.key_beg, (size_t)c.key_len, hipMemcpyDeviceToHost, ctx->stream));
    if (c.prim_len) TSQ_HIP(h, hipMemcpyAsync(primary, m->lprim.as<uint8_t>() + c.prim_beg, (size_t)c.prim_len, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_stats(tsq_mvcc* m, int64_t* scans, int64_t* keys_examined, int64_t* versions_read, int64_t* pairs, double* kernel_ms) {
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    if (scans) *scans = m->scans;
    if (keys_examined) *keys_examined = m->examined;
    if (versions_read) *versions_read = m->walked;
    if (pairs) *pairs = m->pairs;
    if (kernel_ms) *kernel_ms = m->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_cancel(tsq_mvcc* m) {
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    m->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_mvcc_destroy(tsq_mvcc* m) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return;
    (void)hipSetDevice(m->ctx->device);
    (void)hipStreamSynchronize(m->ctx->stream);
    m->hdr.magic = 0;
    delete m;
}
