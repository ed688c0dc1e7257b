// tsq_unionstore.hip — a transaction's merged read on the GPU (gfx950): BufferStore.Get and BufferStore.Iter / IterReverse
// (kv/buffer_store.go:61-99) with kv.UnionIter (kv/union_iter.go:64-152) over the finished transaction buffer (tsq_membuf) as the dirty
// side and the versioned store (tsq_mvcc) read at a startTS as the snapshot side — include/tsq.h "UnionStore"; DESIGN.md §5
// "UnionStore".  The per-position code is tsq_unionstore_dp.h, over tsq_mvcc_dp.h and tsq_memread_dp.h.
//
// tsq_unionstore_scan, merged route:
//   K27a k_un_bounds   : one lane per range — the snapshot interval (tsq_mv_bounds) and the buffer interval (tsq_mr_range_bound twice)
//        tsq_launch_scan64 x 2: the first snapshot and buffer position of every range  (the host reads both totals and the error bits;
//        no buffer position at all: the call goes to tsq_mvcc_scan — the snapshot route)
//   K27b k_un_snapshot : one lane per snapshot position — range, key, lock check (atomicMin of the first locked position), chain walk,
//                        then ONE bound search over the buffer: the slot among the range's candidates, the shadow flag, the keep flag
//   K27c k_un_buffer   : one lane per buffer position — entry, ONE bound search over the store's keys: the slot, the keep flag (PUT),
//                        the skipped and the dangling deletes
//        tsq_launch_scan64 over the keep flags: the pairs before every candidate
//   K27d k_un_prev     : only when a position was locked — the visible snapshot position in front of the first locked one in its range
//                        (atomicMax), every lane one position
//   K27e k_un_decide   : one lane — the lock rule (tsq_un_lock_met) from the ranks, the limit: success or ErrLocked with the lock's fields
//   K27f k_un_place    : one lane per candidate — a kept candidate below the cut writes its source and its two lengths at its ordinal
//        tsq_launch_scan64 x 2: the output offsets and byte totals
//   K27g k_un_rcounts  : one lane per range — its pairs after the limit, from the ranks at its two ends
//        (the host reads the words, the totals and the range counts: second and last synchronisation)
// tsq_unionstore_get:
//   K27h k_un_points   : one lane per key — the buffer first (tsq_mr_point), only a miss or a lock-only entry goes on to the snapshot's
//                        point resolve; keep flag, source, atomicMin of the first key that met a lock
//        scan, K27e (points form), K27f, the two scans  (one synchronisation: the key count sizes everything)
// tsq_unionstore_fetch:
//   K27i k_un_copy     : one lane per pair — its key and value from the side its source names, the offsets, curIsDirty; a cell of the
//                        threshold length (TSQ_KNOB_ROWENC_WAVE_COPY, 64) or more is copied by the whole wave
// Every kernel is a grid-stride loop sized by a count the host knows; every slot and source is checked against its bounds before a
// write or a copy.
#include "tsq_membuf_store.h"
#include "tsq_mvcc_store.h"
#include "tsq_unionstore_dp.h"

#define TSQ_MAGIC_UNIONSTORE 0x74737155u /* 'tsqU' */
#define TSQ_UN_DEFAULT_WAVE_COPY 64

// the words the kernels of one read share and the host reads once at the end
struct UnCtl {
    unsigned long long first_locked;  // atomicMin of the locked snapshot positions (a get: of the keys that met a lock); ~0: none
    unsigned long long prev_visible;  // atomicMax of (visible snapshot position in front of it in its range) + 1; 0: none
    unsigned long long walked, shadowed, dels, dangling, from_buffer;
    int64_t n_pairs, n_fetch, locked;
    int64_t key_beg, key_len, prim_beg, prim_len;
    uint64_t l_start, l_ttl;
    int64_t l_op;
    unsigned int err;
    unsigned int pad;
};

struct UnArgs {
    tsq_mv_store s;
    tsq_mr_buffer b;
    const uint64_t* l_ttl;
    const int64_t* koff;  // per store entry
    const int64_t* voff;
    int64_t s_n;          // store entries
    const uint8_t* rbytes;  // the ranges, or the point keys
    const int64_t* roffs;   // ranges: [2 R + 1]; points: [n + 1] or nullptr
    int64_t rbytes_n, fixed_len;
    int64_t R;       // ranges
    int64_t* slo;    // [R]
    int64_t* sbase;  // [R + 1]: snapshot keys of every range, then (scan) its first snapshot position
    int64_t* blo;    // [R]
    int64_t* bbase;  // [R + 1]: buffer entries of every range, then (scan) its first buffer position
    int64_t S, B, C; // positions of either side; candidates (a get: the keys)
    uint64_t ts;
    int32_t desc;
    int64_t limit;   // INT64_MAX: none
    int64_t M;       // min(C, limit): the most pairs the call can return
    int32_t* chosen; // [S]: the store entry whose pair the snapshot position shows, or -1
    int64_t* ord;    // [C + 1]: keep flags, then (scan) the pairs before every candidate
    int32_t* src;    // [C]: the source of every candidate's pair
    int32_t* sel;    // [M]: the sources of the returned pairs
    int64_t* klens;  // [M + 1]
    int64_t* vlens;  // [M + 1]
    int64_t* rcounts;  // [R]
    uint8_t* found;    // a get: [C]
    UnCtl* ctl;
};

__global__ void __launch_bounds__(256) k_un_bounds(UnArgs a) {
    unsigned int e = 0;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o0 = a.roffs[2 * r], o1 = a.roffs[2 * r + 1], o2 = a.roffs[2 * r + 2];
        int64_t lo = 0, cnt = 0, b0 = 0, b1 = 0;
        if (o0 < 0 || o1 < o0 || o2 < o1 || o2 > a.rbytes_n) {
            e |= TSQ_UN_E_OFFSETS;
        } else {
            tsq_mv_bounds(a.s.k, a.rbytes + o0, o1 - o0, a.rbytes + o1, o2 - o1, 0u, &lo, &cnt);
            uint32_t be = 0;
            b0 = tsq_mr_range_bound(a.b, a.rbytes, a.roffs, 2 * r, &be);
            b1 = tsq_mr_range_bound(a.b, a.rbytes, a.roffs, 2 * r + 1, &be);
        }
        a.slo[r] = lo;
        a.sbase[r] = cnt;
        a.blo[r] = b0;
        a.bbase[r] = tsq_mr_range_count(b0, b1);
    }
    if (e) atomicOr(&a.ctl->err, e);
}

// the candidate slots of range r: [*c0, *c1)
__device__ __forceinline__ void un_slots(const UnArgs& a, int64_t r, int64_t* c0, int64_t* c1) {
    *c0 = a.sbase[r] + a.bbase[r];
    *c1 = a.sbase[r + 1] + a.bbase[r + 1];
}

__global__ void __launch_bounds__(256) k_un_snapshot(UnArgs a) {
    unsigned long long first = ~0ull, shadowed = 0;
    int64_t walked = 0;
    unsigned int err = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.S; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = a.R == 1 ? 0 : tsq_mv_range_of(a.sbase, a.R, p);
        if (r < 0) {  // (no range owns the position: nothing is read)
            a.chosen[p] = -1;
            err |= TSQ_UN_E_INTERNAL;
            continue;
        }
        const int64_t j = p - a.sbase[r];
        const int64_t u = tsq_mv_key_at(a.slo[r], a.sbase[r + 1] - a.sbase[r], j, a.desc);
        int64_t res = -1, slot = -1;
        bool shadow = false;
        if (u >= 0 && u < a.s.k.n) {
            uint64_t ts = a.ts;
            if (tsq_mv_key_lock(a.s, u, &ts)) {
                first = (unsigned long long)p < first ? (unsigned long long)p : first;
            } else {
                const int64_t v0 = a.s.seg[u];
                res = tsq_mv_walk(a.s.cts, a.s.types, v0, v0 + a.s.cnt[u], ts, &walked);
            }
            slot = tsq_un_snapshot_slot(a.b, a.blo[r], a.bbase[r + 1] - a.bbase[r], a.s.k.bytes + a.s.k.beg[u], a.s.k.len[u], j, a.desc, &shadow);
        }
        a.chosen[p] = (int32_t)res;
        int64_t c0 = 0, c1 = 0;
        un_slots(a, r, &c0, &c1);
        if (slot < 0 || c0 + slot >= c1 || c1 > a.C) {
            err |= TSQ_UN_E_INTERNAL;
            continue;
        }
        a.ord[c0 + slot] = tsq_un_keep_snapshot(res, shadow) ? 1 : 0;
        a.src[c0 + slot] = (int32_t)res;
        shadowed += res >= 0 && shadow ? 1ull : 0ull;
    }
    unsigned long long wk = (unsigned long long)walked;
    for (int o = 32; o > 0; o >>= 1) {
        wk += __shfl_xor(wk, o, 64);
        shadowed += __shfl_xor(shadowed, o, 64);
        const unsigned long long f = __shfl_xor(first, o, 64);
        first = f < first ? f : first;
    }
    if ((threadIdx.x & 63) == 0) {
        if (wk) atomicAdd(&a.ctl->walked, wk);
        if (shadowed) atomicAdd(&a.ctl->shadowed, shadowed);
        if (first != ~0ull) atomicMin(&a.ctl->first_locked, first);
    }
    if (err) atomicOr(&a.ctl->err, err);
}

__global__ void __launch_bounds__(256) k_un_buffer(UnArgs a) {
    unsigned long long dels = 0, dangling = 0;
    unsigned int err = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.B; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t r = tsq_mr_range_of(a.bbase, a.R, p);
        const int64_t i = p - a.bbase[r], bcnt = a.bbase[r + 1] - a.bbase[r], scnt = a.sbase[r + 1] - a.sbase[r];
        const int64_t e0 = a.desc ? a.blo[r] + bcnt - 1 - i : a.blo[r] + i;
        if (i < 0 || i >= bcnt || e0 < 0 || e0 >= a.b.m) {  // (the range arrays contradict the buffer's count: nothing is read)
            err |= TSQ_UN_E_INTERNAL;
            continue;
        }
        int64_t e, sj;
        const int64_t slot = tsq_un_buffer_slot(a.b, a.s.k, a.slo[r], scnt, a.blo[r], bcnt, i, a.desc, &e, &sj);
        int64_t c0, c1;
        un_slots(a, r, &c0, &c1);
        if (slot < 0 || c0 + slot >= c1 || c1 > a.C || sj >= scnt) {
            err |= TSQ_UN_E_INTERNAL;
            continue;
        }
        const uint8_t op = a.b.oops[e];
        a.ord[c0 + slot] = tsq_un_keep_buffer(op) ? 1 : 0;
        a.src[c0 + slot] = tsq_un_src_buffer(e);
        if (op == TSQ_MVCC_OP_DEL) {
            dels++;
            dangling += sj < 0 || a.chosen[a.sbase[r] + sj] < 0 ? 1ull : 0ull;  // (k_un_snapshot ran before this kernel on the stream)
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        dels += __shfl_xor(dels, o, 64);
        dangling += __shfl_xor(dangling, o, 64);
    }
    if ((threadIdx.x & 63) == 0) {
        if (dels) atomicAdd(&a.ctl->dels, dels);
        if (dangling) atomicAdd(&a.ctl->dangling, dangling);
    }
    if (err) atomicOr(&a.ctl->err, err);
}

__global__ void __launch_bounds__(256) k_un_prev(UnArgs a) {
    const unsigned long long L = a.ctl->first_locked;
    if (L >= (unsigned long long)a.S) return;  // (uniform: no position was locked)
    const int64_t r = tsq_mv_range_of(a.sbase, a.R, (int64_t)L);
    if (r < 0) return;
    unsigned long long best = 0;
    for (int64_t q = a.sbase[r] + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; q < (int64_t)L; q += (int64_t)gridDim.x * blockDim.x)
        if (a.chosen[q] >= 0) best = (unsigned long long)q + 1;  // (q grows along the loop)
    for (int o = 32; o > 0; o >>= 1) {
        const unsigned long long f = __shfl_xor(best, o, 64);
        best = f > best ? f : best;
    }
    if ((threadIdx.x & 63) == 0 && best) atomicMax(&a.ctl->prev_visible, best);
}

__device__ __forceinline__ void un_lock_fields(const UnArgs& a, UnCtl* c, int64_t u) {
    if (u < 0 || u >= a.s.k.n) return;
    const int32_t j = a.s.lock[u];  // (>= 0: the key was locked)
    if (j < 0) return;
    c->key_beg = a.s.k.beg[u];
    c->key_len = a.s.k.len[u];
    c->prim_beg = a.s.l_poff[j];
    c->prim_len = a.s.l_poff[j + 1] - a.s.l_poff[j];
    c->l_start = a.s.l_start[j];
    c->l_ttl = a.l_ttl[j];
    c->l_op = a.s.l_op[j];
}
// points = 1: candidate i is key i, the first key that met a lock fails the call
__global__ void __launch_bounds__(64) k_un_decide(UnArgs a, int points) {
    if (threadIdx.x != 0) return;
    UnCtl* c = a.ctl;
    const int64_t T = a.ord[a.C];
    const int64_t Tm = T < a.M ? T : a.M;
    const unsigned long long L = c->first_locked;
    c->locked = 0;
    c->n_pairs = c->n_fetch = Tm;
    if (points) {
        if (L < (unsigned long long)a.C) {
            c->locked = 1;
            c->n_pairs = a.ord[L];
            c->n_fetch = 0;
            un_lock_fields(a, c, (int64_t)a.src[L]);  // (k_un_points left the key's ordinal there)
        }
        return;
    }
    if (L >= (unsigned long long)a.S) return;
    const int64_t r = tsq_mv_range_of(a.sbase, a.R, (int64_t)L);
    if (r < 0) return;
    const int64_t sb = a.sbase[r], scnt = a.sbase[r + 1] - sb;
    int64_t c0, c1;
    un_slots(a, r, &c0, &c1);
    const unsigned long long pv = c->prev_visible;
    const bool has_prev = pv > (unsigned long long)sb && pv <= L;
    int64_t before_prev = 0;
    bool shadow = false;
    if (has_prev) {
        const int64_t j = (int64_t)pv - 1 - sb, u = tsq_mv_key_at(a.slo[r], scnt, j, a.desc);
        const int64_t slot = tsq_un_snapshot_slot(a.b, a.blo[r], a.bbase[r + 1] - a.bbase[r], a.s.k.bytes + a.s.k.beg[u], a.s.k.len[u], j, a.desc, &shadow);
        before_prev = a.ord[c0 + slot < c1 ? c0 + slot : c0];
    }
    int64_t np = 0;
    if (tsq_un_lock_met(has_prev, before_prev, shadow, a.ord[c0], a.limit, &np)) {
        c->locked = 1;
        c->n_pairs = np;
        c->n_fetch = 0;
        un_lock_fields(a, c, tsq_mv_key_at(a.slo[r], scnt, (int64_t)L - sb, a.desc));
    }
}

__global__ void __launch_bounds__(256) k_un_place(UnArgs a) {
    const int64_t n = a.ctl->n_fetch;
    unsigned long long fb = 0;
    for (int64_t c = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; c < a.C; c += (int64_t)gridDim.x * blockDim.x) {
        const int64_t o = a.ord[c];
        if (a.ord[c + 1] == o || o < 0 || o >= n || o >= a.M) continue;
        const int32_t s = a.src[c];
        const int64_t e = tsq_un_src_entry(s);
        if (e >= (tsq_un_src_is_buffer(s) ? a.b.m : a.s_n)) continue;  // (checked, not assumed: the pair keeps a length of 0)
        a.sel[o] = s;
        if (tsq_un_src_is_buffer(s)) {
            a.klens[o] = a.b.okoff[e + 1] - a.b.okoff[e];
            a.vlens[o] = a.b.ovoff[e + 1] - a.b.ovoff[e];
            fb++;
        } else {
            a.klens[o] = a.koff[e + 1] - a.koff[e];
            a.vlens[o] = a.voff[e + 1] - a.voff[e];
        }
    }
    for (int o = 32; o > 0; o >>= 1) fb += __shfl_xor(fb, o, 64);
    if ((threadIdx.x & 63) == 0 && fb) atomicAdd(&a.ctl->from_buffer, fb);
}
__global__ void __launch_bounds__(256) k_un_rcounts(UnArgs a) {
    const int64_t n = a.ctl->n_fetch;
    for (int64_t r = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; r < a.R; r += (int64_t)gridDim.x * blockDim.x) {
        int64_t c0, c1;
        un_slots(a, r, &c0, &c1);
        c0 = c0 < 0 ? 0 : (c0 > a.C ? a.C : c0);  // (a scan of counts stays inside their sum: checked, not assumed)
        c1 = c1 < c0 ? c0 : (c1 > a.C ? a.C : c1);
        const int64_t x = a.ord[c0], z = a.ord[c1];
        a.rcounts[r] = (z < n ? z : n) - (x < n ? x : n);
    }
}

__global__ void __launch_bounds__(256) k_un_points(UnArgs a) {
    unsigned long long first = ~0ull;
    int64_t walked = 0;
    unsigned int err = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.C; i += (int64_t)gridDim.x * blockDim.x) {
        int64_t src = -1;
        const int v = tsq_un_point(a.b, a.s, a.rbytes, a.roffs, a.fixed_len, a.rbytes_n, i, a.ts, &src, &walked, &err);
        const bool keep = v == TSQ_UN_PT_BUFFER || v == TSQ_UN_PT_SNAPSHOT;
        a.ord[i] = keep ? 1 : 0;
        a.src[i] = v == TSQ_UN_PT_BUFFER ? tsq_un_src_buffer(src) : (int32_t)src;
        a.found[i] = keep ? 1 : 0;
        if (v == TSQ_UN_PT_LOCKED) first = (unsigned long long)i < first ? (unsigned long long)i : first;
    }
    unsigned long long wk = (unsigned long long)walked;
    for (int o = 32; o > 0; o >>= 1) {
        wk += __shfl_xor(wk, o, 64);
        const unsigned long long f = __shfl_xor(first, o, 64);
        first = f < first ? f : first;
    }
    if ((threadIdx.x & 63) == 0) {
        if (wk) atomicAdd(&a.ctl->walked, wk);
        if (first != ~0ull) atomicMin(&a.ctl->first_locked, first);
    }
    if (err) atomicOr(&a.ctl->err, err);
}

struct UnCopyArgs {
    const uint8_t* skeys;  // the store
    const int64_t* skoff;
    const uint8_t* svals;
    const int64_t* svoff;
    int64_t s_n, skey_bytes, sval_bytes;
    const uint8_t* bkeys;  // the buffer
    const int64_t* bkoff;
    const uint8_t* bvals;
    const int64_t* bvoff;
    int64_t b_m, bkey_bytes, bval_bytes;
    const int32_t* sel;
    const int64_t* klens;  // scanned: the output offsets
    const int64_t* vlens;
    int64_t n, key_bytes, value_bytes, wave_copy;
    uint8_t* keys;
    int64_t* key_offsets;
    uint8_t* values;
    int64_t* value_offsets;
    uint8_t* from_buffer;
};
// every lane of the wave brings one cell (len 0: none): short cells by their lane, long ones by the whole wave, one after the other
__device__ __forceinline__ void un_copy_cells(int lane, const uint8_t* s, uint8_t* d, int64_t len, int64_t wave_copy) {
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
__global__ void __launch_bounds__(256) k_un_copy(UnCopyArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    if (blockIdx.x == 0 && threadIdx.x == 0) {
        a.key_offsets[a.n] = a.key_bytes;
        a.value_offsets[a.n] = a.value_bytes;
    }
    for (int64_t p0 = wave * 64; p0 < a.n; p0 += nwaves * 64) {  // (wave uniform)
        const int64_t o = p0 + lane;
        int64_t kl = 0, vl = 0;
        const uint8_t* ks = a.skeys;
        const uint8_t* vs = a.svals;
        uint8_t* kd = a.keys;
        uint8_t* vd = a.values;
        if (o < a.n) {
            const int32_t s = a.sel[o];
            const bool fb = tsq_un_src_is_buffer(s);
            const int64_t e = tsq_un_src_entry(s);
            const int64_t dk = a.klens[o], dv = a.vlens[o], l0 = a.klens[o + 1] - dk, l1 = a.vlens[o + 1] - dv;
            if (e >= 0 && e < (fb ? a.b_m : a.s_n)) {
                const int64_t sk = fb ? a.bkoff[e] : a.skoff[e], sv = fb ? a.bvoff[e] : a.svoff[e];
                if (l0 >= 0 && l1 >= 0 && sk >= 0 && sk + l0 <= (fb ? a.bkey_bytes : a.skey_bytes) && sv >= 0 && sv + l1 <= (fb ? a.bval_bytes : a.sval_bytes) &&
                    dk >= 0 && dk + l0 <= a.key_bytes && dv >= 0 && dv + l1 <= a.value_bytes) {
                    kl = l0, vl = l1;
                    ks = (fb ? a.bkeys : a.skeys) + sk, vs = (fb ? a.bvals : a.svals) + sv, kd += dk, vd += dv;
                }
            }
            a.key_offsets[o] = dk;
            a.value_offsets[o] = dv;
            if (a.from_buffer) a.from_buffer[o] = fb ? 1 : 0;
        }
        un_copy_cells(lane, ks, kd, kl, a.wave_copy);
        un_copy_cells(lane, vs, vd, vl, a.wave_copy);
    }
}

// ====================================================================== host side
struct tsq_unionstore {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    std::atomic<int> cancelled{0};
    tsq_mvcc* store = nullptr;  // borrowed
    tsq_membuf* mb = nullptr;   // borrowed; may be NULL
    uint64_t ts = 0;
    // one read
    DevBuf rng, roff, slo, sbase, blo, bbase, chosen, ord, src, sel, klens, vlens, rcounts, found, scan_tmp, ctl;
    UnCtl last;
    bool have_last = false;
    int32_t last_route = TSQ_UNION_ROUTE_NONE;
    int64_t last_pairs = 0, last_key_bytes = 0, last_value_bytes = 0, last_finishes = 0;
    int64_t last_store_scans = 0;  // the snapshot route: the store's scan count behind this handle's scan — another scan of the store takes its place
    int64_t scans = 0, merged = 0, snapshot_only = 0, gets = 0, pairs = 0;
    double kernel_ms = 0;
    DevEvent ev[2];
};

namespace {
tsq_status un_enter(tsq_unionstore* us, tsq_unionstore_result* result) {
    tsq_handle_hdr* h = &us->hdr;
    if (result) memset(result, 0, sizeof *result);
    us->have_last = false;  // whatever becomes of this read, the last one can no longer be fetched
    us->last_route = TSQ_UNION_ROUTE_NONE;
    if (us->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "union store cancelled");
    if (!result) return tsq_fail(h, TSQ_ERR_INVALID, "union store: NULL result");
    if (us->mb && !us->mb->finished) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: not finished");
    TSQ_HIP(h, hipSetDevice(us->ctx->device));
    return TSQ_OK;
}
// the caller's array on the device: its own, or a copy in `own`
tsq_status un_dev_array(tsq_unionstore* us, DevBuf& own, const void* src, size_t bytes, bool dev, const void** out) {
    *out = src;
    if (dev || !src || !bytes) return TSQ_OK;
    TSQ_TRY(own.reserve(us->ctx, &us->hdr, bytes + 64));
    TSQ_HIP(&us->hdr, hipMemcpyAsync(own.p, src, bytes, hipMemcpyHostToDevice, us->ctx->stream));
    *out = own.p;
    return TSQ_OK;
}
void un_views(tsq_unionstore* us, UnArgs* a) {
    tsq_mv_store_view(us->store, &a->s);
    a->l_ttl = us->store->lttl.as<uint64_t>();
    a->koff = us->store->koff.as<int64_t>();
    a->voff = us->store->voff.as<int64_t>();
    a->s_n = us->store->n;
    memset(&a->b, 0, sizeof a->b);
    if (us->mb) {
        a->b.okeys = us->mb->okeys.as<uint8_t>();
        a->b.okoff = us->mb->okoff.as<int64_t>();
        a->b.oops = us->mb->oops.as<uint8_t>();
        a->b.ovoff = us->mb->ovoff.as<int64_t>();
        a->b.m = us->mb->m;
    }
    a->ts = us->ts;
}
tsq_status un_ctl_init(tsq_unionstore* us, UnArgs* a) {
    TSQ_TRY(us->ctl.reserve(us->ctx, &us->hdr, sizeof(UnCtl) + 64));
    a->ctl = us->ctl.as<UnCtl>();
    TSQ_HIP(&us->hdr, hipMemsetAsync(a->ctl, 0, sizeof(UnCtl), us->ctx->stream));
    TSQ_HIP(&us->hdr, hipMemsetAsync(&a->ctl->first_locked, 0xff, 8, us->ctx->stream));
    return TSQ_OK;
}
// the snapshot route: tsq_mvcc_scan on the borrowed store; host ranges
tsq_status un_snapshot_route(tsq_unionstore* us, const uint8_t* range_bytes, const int64_t* range_offsets, int64_t R, int32_t desc, int64_t limit,
                             tsq_unionstore_result* result, int64_t* range_counts) {
    tsq_handle_hdr* h = &us->hdr;
    tsq_mvcc_result mr;
    memset(&mr, 0, sizeof mr);
    us->last_route = TSQ_UNION_ROUTE_SNAPSHOT;
    us->snapshot_only++;
    const tsq_status st = tsq_mvcc_scan(us->store, range_bytes, range_offsets, nullptr, R, us->ts, desc, limit, &mr, range_counts);
    result->n_pairs = mr.n_pairs;
    us->last_store_scans = us->store->scans;
    if (st == TSQ_ERR_LOCKED) {
        memset(&us->last, 0, sizeof us->last);
        us->last.locked = 1;
        us->have_last = true;
        return tsq_fail(h, st, "union store: key is locked");
    }
    if (st != TSQ_OK) return tsq_fail(h, st, us->store->hdr.err);
    result->key_bytes = mr.key_bytes;
    result->value_bytes = mr.value_bytes;
    result->positions_snapshot = mr.positions;
    memset(&us->last, 0, sizeof us->last);
    us->last_pairs = mr.n_pairs, us->last_key_bytes = mr.key_bytes, us->last_value_bytes = mr.value_bytes;
    us->pairs += mr.n_pairs;
    us->have_last = true;
    return TSQ_OK;
}
// behind the keep flags: scan, decide, place, lengths -> offsets; the host reads everything once
tsq_status un_finish(tsq_unionstore* us, UnArgs& a, int points, tsq_unionstore_result* result, int64_t* range_counts, uint8_t* found) {
    tsq_handle_hdr* h = &us->hdr;
    tsq_ctx* ctx = us->ctx;
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.ord, a.C, us->scan_tmp));
    if (!points) hipLaunchKernelGGL(k_un_prev, dim3(tsq_grid_for(ctx, a.S, 256)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_un_decide, dim3(1), dim3(64), 0, ctx->stream, a, points);
    TSQ_HIP(h, hipMemsetAsync(a.klens, 0, ((size_t)a.M + 1) * 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(a.vlens, 0, ((size_t)a.M + 1) * 8, ctx->stream));
    hipLaunchKernelGGL(k_un_place, dim3(tsq_grid_for(ctx, a.C, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.klens, a.M, us->scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.vlens, a.M, us->scan_tmp));
    if (!points && range_counts) {
        hipLaunchKernelGGL(k_un_rcounts, dim3(tsq_grid_for(ctx, a.R, 256)), dim3(256), 0, ctx->stream, a);
        TSQ_HIP(h, hipGetLastError());
        TSQ_HIP(h, hipMemcpyAsync(range_counts, a.rcounts, (size_t)a.R * 8, hipMemcpyDeviceToHost, ctx->stream));
    }
    TSQ_HIP(h, hipEventRecord(us->ev[1], ctx->stream));
    int64_t kb = 0, vb = 0;
    TSQ_HIP(h, hipMemcpyAsync(&us->last, a.ctl, sizeof(UnCtl), hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&kb, a.klens + a.M, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&vb, a.vlens + a.M, 8, hipMemcpyDeviceToHost, ctx->stream));
    if (points && found) TSQ_HIP(h, hipMemcpyAsync(found, a.found, (size_t)a.C, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // the counts and the status
    float ms = 0;
    if (hipEventElapsedTime(&ms, us->ev[0], us->ev[1]) == hipSuccess) us->kernel_ms += ms;
    const UnCtl& c = us->last;
    if (c.err & TSQ_UN_E_OFFSETS) return tsq_fail(h, TSQ_ERR_INVALID, "union store: offsets decrease or leave their buffer");
    if (c.err) return tsq_fail(h, TSQ_ERR_HIP, "internal: a candidate of the union read left its range's slots");
    result->n_pairs = c.n_pairs;
    if (c.locked) {
        if (range_counts) memset(range_counts, 0, (size_t)a.R * 8);
        if (points && found) memset(found, 0, (size_t)a.C);
        us->have_last = true;  // (for tsq_unionstore_locked; nothing to fetch)
        return tsq_fail(h, TSQ_ERR_LOCKED, "union store: key is locked");
    }
    if (c.n_pairs < 0 || c.n_pairs > a.M || c.n_fetch != c.n_pairs || kb < 0 || vb < 0 || (int64_t)c.from_buffer > c.n_pairs)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the counts of the union read are out of range");
    result->key_bytes = kb;
    result->value_bytes = vb;
    result->shadowed = (int64_t)c.shadowed;
    result->skipped_dels = (int64_t)c.dels;
    result->dangling_dels = (int64_t)c.dangling;
    result->from_buffer = (int64_t)c.from_buffer;
    us->last_pairs = c.n_pairs, us->last_key_bytes = kb, us->last_value_bytes = vb;
    us->last_finishes = us->mb ? us->mb->finishes : 0;
    us->pairs += c.n_pairs;
    us->have_last = true;
    return TSQ_OK;
}
tsq_status un_reserve_candidates(tsq_unionstore* us, UnArgs& a) {
    tsq_handle_hdr* h = &us->hdr;
    tsq_ctx* ctx = us->ctx;
    TSQ_TRY(us->ord.reserve(ctx, h, ((size_t)a.C + 1) * 8 + 64));
    TSQ_TRY(us->src.reserve(ctx, h, (size_t)a.C * 4 + 64));
    TSQ_TRY(us->sel.reserve(ctx, h, (size_t)a.M * 4 + 64));
    TSQ_TRY(us->klens.reserve(ctx, h, ((size_t)a.M + 1) * 8 + 64));
    TSQ_TRY(us->vlens.reserve(ctx, h, ((size_t)a.M + 1) * 8 + 64));
    a.ord = us->ord.as<int64_t>(), a.src = us->src.as<int32_t>(), a.sel = us->sel.as<int32_t>();
    a.klens = us->klens.as<int64_t>(), a.vlens = us->vlens.as<int64_t>();
    return TSQ_OK;
}
}  // namespace

TSQ_API tsq_status tsq_unionstore_create(tsq_ctx* ctx, tsq_mvcc* store, tsq_membuf* mb, uint64_t start_ts, tsq_unionstore** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !out || !store) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_unionstore_create: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (store->hdr.magic != TSQ_MAGIC_MVCC || (mb && mb->hdr.magic != TSQ_MAGIC_MEMBUF)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_unionstore_create: not a store or not a buffer");
    if (store->ctx != ctx || (mb && mb->ctx != ctx)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_unionstore_create: the store and the buffer must belong to the context");
    std::unique_ptr<tsq_unionstore> us(new tsq_unionstore());
    us->hdr.magic = TSQ_MAGIC_UNIONSTORE;
    us->ctx = ctx;
    us->store = store;
    us->mb = mb;
    us->ts = start_ts;
    memset(&us->last, 0, sizeof us->last);
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    for (int i = 0; i < 2; i++)
        if (us->ev[i].create() != hipSuccess) return tsq_fail(ch, TSQ_ERR_HIP, "hipEventCreate");
    *out = us.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionstore_scan(tsq_unionstore* us, const uint8_t* range_bytes, const int64_t* range_offsets, int64_t n_ranges, uint32_t data_flags,
                                       int32_t desc, int64_t limit, tsq_unionstore_result* result, int64_t* range_counts) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(us, TSQ_MAGIC_UNIONSTORE));
    if (!us || us->hdr.magic != TSQ_MAGIC_UNIONSTORE) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &us->hdr;
    TSQ_TRY(un_enter(us, result));
    const int64_t R = n_ranges;
    if (R < 0) return tsq_fail(h, TSQ_ERR_INVALID, "union store: negative count");
    if (R > 0 && !range_offsets) return tsq_fail(h, TSQ_ERR_INVALID, "union store: NULL array");
    if (R >= (1LL << 30)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "union store: 2^30 ranges or more");
    tsq_ctx* ctx = us->ctx;
    const bool dev = data_flags & TSQ_COL_DEVICE;
    us->scans++;
    if (range_counts && R > 0) memset(range_counts, 0, (size_t)R * 8);
    // the ranges on both sides of the bus: a device caller's are read back once (the snapshot route takes host ranges, and the copy
    // below is sized by the last offset either way)
    std::vector<int64_t> h_offs;
    std::vector<uint8_t> h_bytes;
    int64_t rb_n = 0;
    if (R > 0 && dev) {
        h_offs.resize((size_t)2 * R + 1);
        TSQ_HIP(h, hipMemcpy(h_offs.data(), range_offsets, h_offs.size() * 8, hipMemcpyDeviceToHost));
    }
    const int64_t* offs_host = dev ? h_offs.data() : range_offsets;
    if (R > 0) {
        for (int64_t j = 0; j < 2 * R; j++)
            if (offs_host[j] < 0 || offs_host[j] > offs_host[j + 1]) return tsq_fail(h, TSQ_ERR_INVALID, "union store: offsets decrease or leave their buffer");
        rb_n = offs_host[2 * R];
        if (rb_n > 0 && !range_bytes) return tsq_fail(h, TSQ_ERR_INVALID, "union store: NULL array");
    }
    auto snapshot_route = [&]() -> tsq_status {
        const uint8_t* hb = range_bytes;
        if (dev && rb_n > 0) {
            h_bytes.resize((size_t)rb_n);
            TSQ_HIP(h, hipMemcpy(h_bytes.data(), range_bytes, (size_t)rb_n, hipMemcpyDeviceToHost));
            hb = h_bytes.data();
        }
        return un_snapshot_route(us, hb, offs_host, R, desc, limit, result, range_counts);
    };
    if (!us->mb || us->mb->m == 0 || R == 0 || limit == 0) return snapshot_route();  // (nothing to merge, or nothing to examine)
    UnArgs a;
    memset(&a, 0, sizeof a);
    un_views(us, &a);
    const void* d_bytes = nullptr;
    const void* d_offs = nullptr;
    TSQ_TRY(un_dev_array(us, us->rng, range_bytes, (size_t)rb_n, dev, &d_bytes));
    TSQ_TRY(un_dev_array(us, us->roff, range_offsets, ((size_t)2 * R + 1) * 8, dev, &d_offs));
    a.rbytes = (const uint8_t*)d_bytes, a.roffs = (const int64_t*)d_offs, a.rbytes_n = rb_n, a.R = R;
    a.desc = desc ? 1 : 0;
    a.limit = limit < 0 ? INT64_MAX : limit;
    for (DevBuf* b : {&us->slo, &us->blo, &us->rcounts}) TSQ_TRY(b->reserve(ctx, h, (size_t)R * 8 + 64));
    for (DevBuf* b : {&us->sbase, &us->bbase}) TSQ_TRY(b->reserve(ctx, h, ((size_t)R + 1) * 8 + 64));
    a.slo = us->slo.as<int64_t>(), a.sbase = us->sbase.as<int64_t>(), a.blo = us->blo.as<int64_t>(), a.bbase = us->bbase.as<int64_t>();
    a.rcounts = us->rcounts.as<int64_t>();
    TSQ_TRY(un_ctl_init(us, &a));
    TSQ_HIP(h, hipEventRecord(us->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_un_bounds, dim3(tsq_grid_for(ctx, R, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.sbase, R, us->scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.bbase, R, us->scan_tmp));
    int64_t S = 0, B = 0;
    unsigned int rerr = 0;
    TSQ_HIP(h, hipMemcpyAsync(&S, a.sbase + R, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&B, a.bbase + R, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&rerr, &a.ctl->err, 4, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // the position totals size the per-position buffers
    if (rerr) return tsq_fail(h, TSQ_ERR_INVALID, "union store: offsets decrease or leave their buffer");
    if (S < 0 || B < 0 || S > us->store->U * R || B > us->mb->m * R) return tsq_fail(h, TSQ_ERR_HIP, "internal: the position counts of the union read are out of range");
    if (S + B >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "union store: 2^31 scan positions or more");
    if (B == 0) return snapshot_route();  // no range holds a buffer entry
    us->last_route = TSQ_UNION_ROUTE_MERGE;
    us->merged++;
    result->positions_snapshot = S;
    result->positions_buffer = B;
    a.S = S, a.B = B, a.C = S + B;
    a.M = std::min<int64_t>(a.C, a.limit);
    TSQ_TRY(us->chosen.reserve(ctx, h, (size_t)S * 4 + 64));
    a.chosen = us->chosen.as<int32_t>();
    TSQ_TRY(un_reserve_candidates(us, a));
    if (S > 0) hipLaunchKernelGGL(k_un_snapshot, dim3(tsq_grid_for(ctx, S, 256)), dim3(256), 0, ctx->stream, a);
    hipLaunchKernelGGL(k_un_buffer, dim3(tsq_grid_for(ctx, B, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    return un_finish(us, a, 0, result, range_counts, nullptr);
}

TSQ_API tsq_status tsq_unionstore_get(tsq_unionstore* us, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n, uint32_t data_flags,
                                      tsq_unionstore_result* result, uint8_t* found) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(us, TSQ_MAGIC_UNIONSTORE));
    if (!us || us->hdr.magic != TSQ_MAGIC_UNIONSTORE) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &us->hdr;
    TSQ_TRY(un_enter(us, result));
    if (n < 0 || key_bytes < 0) return tsq_fail(h, TSQ_ERR_INVALID, "union store: negative count");
    if (n > 0 && key_bytes > 0 && !keys) return tsq_fail(h, TSQ_ERR_INVALID, "union store: NULL array");
    if (n > 0 && !key_offsets && key_bytes % n != 0) return tsq_fail(h, TSQ_ERR_INVALID, "union store: keys of a fixed length need key_bytes to be a multiple of n");
    if (n >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "union store: 2^31 scan positions or more");
    tsq_ctx* ctx = us->ctx;
    const bool dev = data_flags & TSQ_COL_DEVICE;
    us->gets++;
    us->last_route = TSQ_UNION_ROUTE_POINTS;
    if (found && n > 0) memset(found, 0, (size_t)n);
    if (n == 0) {
        memset(&us->last, 0, sizeof us->last);
        us->last_pairs = us->last_key_bytes = us->last_value_bytes = 0;
        us->last_finishes = us->mb ? us->mb->finishes : 0;
        us->have_last = true;
        return TSQ_OK;
    }
    UnArgs a;
    memset(&a, 0, sizeof a);
    un_views(us, &a);
    const void* d_bytes = nullptr;
    const void* d_offs = nullptr;
    TSQ_TRY(un_dev_array(us, us->rng, keys, (size_t)key_bytes, dev, &d_bytes));
    TSQ_TRY(un_dev_array(us, us->roff, key_offsets, ((size_t)n + 1) * 8, dev, &d_offs));
    a.rbytes = (const uint8_t*)d_bytes, a.roffs = (const int64_t*)d_offs, a.rbytes_n = key_bytes;
    a.fixed_len = key_offsets ? 0 : key_bytes / n;
    a.limit = INT64_MAX;
    a.C = a.M = n;
    result->positions_snapshot = result->positions_buffer = n;
    TSQ_TRY(un_reserve_candidates(us, a));
    TSQ_TRY(us->found.reserve(ctx, h, (size_t)n + 64));
    a.found = us->found.as<uint8_t>();
    TSQ_TRY(un_ctl_init(us, &a));
    TSQ_HIP(h, hipEventRecord(us->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_un_points, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    return un_finish(us, a, 1, result, nullptr, found);
}

TSQ_API tsq_status tsq_unionstore_fetch(tsq_unionstore* us, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* values, int64_t value_cap,
                                        int64_t* value_offsets, uint8_t* from_buffer) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(us, TSQ_MAGIC_UNIONSTORE));
    if (!us || us->hdr.magic != TSQ_MAGIC_UNIONSTORE) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &us->hdr;
    if (us->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "union store cancelled");
    if (!us->have_last || us->last.locked) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_unionstore_fetch: no successful read to fetch");
    if (!key_offsets || !value_offsets || key_cap < 0 || value_cap < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_unionstore_fetch: bad arguments");
    if (key_cap < us->last_key_bytes || value_cap < us->last_value_bytes || (us->last_key_bytes > 0 && !keys) || (us->last_value_bytes > 0 && !values))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_unionstore_fetch: output buffer too small");
    tsq_ctx* ctx = us->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const int64_t n = us->last_pairs;
    if (us->last_route == TSQ_UNION_ROUTE_SNAPSHOT) {
        if (us->store->scans != us->last_store_scans) return tsq_fail(h, TSQ_ERR_INVALID, "union store: the store was scanned since this handle's read");
        const tsq_status st = tsq_mvcc_fetch(us->store, keys, key_cap, key_offsets, values, value_cap, value_offsets);
        if (st != TSQ_OK) return tsq_fail(h, st, us->store->hdr.err);
        if (from_buffer && n > 0) {
            TSQ_HIP(h, hipMemsetAsync(from_buffer, 0, (size_t)n, ctx->stream));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        }
        return TSQ_OK;
    }
    if (us->mb && (!us->mb->finished || us->mb->finishes != us->last_finishes)) return tsq_fail(h, TSQ_ERR_INVALID, "membuf: not finished");
    if (n == 0) {
        TSQ_HIP(h, hipMemsetAsync(key_offsets, 0, 8, ctx->stream));
        TSQ_HIP(h, hipMemsetAsync(value_offsets, 0, 8, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        return TSQ_OK;
    }
    UnCopyArgs c;
    memset(&c, 0, sizeof c);
    const tsq_mvcc* m = us->store;
    c.skeys = m->keys.as<uint8_t>(), c.skoff = m->koff.as<int64_t>(), c.svals = m->vals.as<uint8_t>(), c.svoff = m->voff.as<int64_t>();
    c.s_n = m->n, c.skey_bytes = m->key_bytes, c.sval_bytes = m->value_bytes;
    if (us->mb) {
        const tsq_membuf* b = us->mb;
        c.bkeys = b->okeys.as<uint8_t>(), c.bkoff = b->okoff.as<int64_t>(), c.bvals = b->ovals.as<uint8_t>(), c.bvoff = b->ovoff.as<int64_t>();
        c.b_m = b->m, c.bkey_bytes = b->okey_bytes, c.bval_bytes = b->oval_bytes;
    }
    c.sel = us->sel.as<int32_t>(), c.klens = us->klens.as<int64_t>(), c.vlens = us->vlens.as<int64_t>();
    c.n = n, c.key_bytes = us->last_key_bytes, c.value_bytes = us->last_value_bytes;
    c.wave_copy = tsq_knob(ctx, TSQ_KNOB_ROWENC_WAVE_COPY, TSQ_UN_DEFAULT_WAVE_COPY);
    c.keys = keys, c.key_offsets = key_offsets, c.values = values, c.value_offsets = value_offsets, c.from_buffer = from_buffer;
    hipLaunchKernelGGL(k_un_copy, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, c);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionstore_locked(tsq_unionstore* us, uint8_t* key, int64_t key_cap, int64_t* key_len, uint8_t* primary, int64_t primary_cap,
                                         int64_t* primary_len, uint64_t* start_ts, uint64_t* ttl, int32_t* op) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(us, TSQ_MAGIC_UNIONSTORE));
    if (!us || us->hdr.magic != TSQ_MAGIC_UNIONSTORE) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &us->hdr;
    if (us->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "union store cancelled");
    if (!us->have_last || !us->last.locked) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_unionstore_locked: the last read met no lock");
    tsq_mvcc* m = us->store;
    if (us->last_route == TSQ_UNION_ROUTE_SNAPSHOT) {
        if (m->scans != us->last_store_scans) return tsq_fail(h, TSQ_ERR_INVALID, "union store: the store was scanned since this handle's read");
        const tsq_status st = tsq_mvcc_locked(m, key, key_cap, key_len, primary, primary_cap, primary_len, start_ts, ttl, op);
        if (st != TSQ_OK) return tsq_fail(h, st, m->hdr.err);
        return TSQ_OK;
    }
    const UnCtl& c = us->last;
    if (c.key_len < 0 || c.key_beg < 0 || c.key_beg + c.key_len > m->key_bytes + m->lkey_bytes || c.prim_len < 0 || c.prim_beg < 0 ||
        c.prim_beg + c.prim_len > m->lprim_bytes)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the lock of the union read is out of range");
    if (key_len) *key_len = c.key_len;
    if (primary_len) *primary_len = c.prim_len;
    if (start_ts) *start_ts = c.l_start;
    if (ttl) *ttl = c.l_ttl;
    if (op) *op = (int32_t)c.l_op;
    if (key_cap < c.key_len || primary_cap < c.prim_len || (c.key_len > 0 && !key) || (c.prim_len > 0 && !primary))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_unionstore_locked: buffer too small (the lengths are filled in)");
    tsq_ctx* ctx = us->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    if (c.key_len) TSQ_HIP(h, hipMemcpyAsync(key, m->keys.as<uint8_t>() + c.key_beg, (size_t)c.key_len, hipMemcpyDeviceToHost, ctx->stream));
    if (c.prim_len) TSQ_HIP(h, hipMemcpyAsync(primary, m->lprim.as<uint8_t>() + c.prim_beg, (size_t)c.prim_len, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionstore_stats(tsq_unionstore* us, int64_t* scans, int64_t* merged, int64_t* snapshot_only, int64_t* gets, int64_t* pairs,
                                        int32_t* last_route, double* kernel_ms) {
    if (!us || us->hdr.magic != TSQ_MAGIC_UNIONSTORE) return TSQ_ERR_INVALID;
    if (scans) *scans = us->scans;
    if (merged) *merged = us->merged;
    if (snapshot_only) *snapshot_only = us->snapshot_only;
    if (gets) *gets = us->gets;
    if (pairs) *pairs = us->pairs;
    if (last_route) *last_route = us->last_route;
    if (kernel_ms) *kernel_ms = us->kernel_ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_unionstore_cancel(tsq_unionstore* us) {
    if (!us || us->hdr.magic != TSQ_MAGIC_UNIONSTORE) return TSQ_ERR_INVALID;
    us->cancelled.store(1);
    return TSQ_OK;
}

TSQ_API void tsq_unionstore_destroy(tsq_unionstore* us) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(us, TSQ_MAGIC_UNIONSTORE));
    if (!us || us->hdr.magic != TSQ_MAGIC_UNIONSTORE) return;
    (void)hipSetDevice(us->ctx->device);
    (void)hipStreamSynchronize(us->ctx->stream);
    us->hdr.magic = 0;
    delete us;
}
