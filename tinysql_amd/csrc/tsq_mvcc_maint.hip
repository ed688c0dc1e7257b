// tsq_mvcc_maint.hip — the range calls of an MVCC store on the GPU (gfx950): ScanLock, ResolveLock / BatchResolveLock, GC and
// DeleteRange of the reference's MVCCLevelDB (store/mockstore/mocktikv/mvcc_leveldb.go:906-1090) over a tsq_mvcc store in HBM
// (include/tsq.h "MVCC lock resolution and GC").  The per-lock, per-key and per-entry code is tsq_mvcc_maint_dp.h.  Each
// call is one pass over a key range with one decision per lock or per version; what changes the store goes through the apply of the
// writes (tsq_mw_apply, tsq_mvcc_write.hip) into the NEXT store.
//
// every call:
//   K23a k_mm_bounds    : one lane — the range as bounds in the key universe, among the version entries and among the locks (four
//                         bound searches), the ordinals of the first and the last key with versions
//        (the host reads the bounds: they size the passes below)
// tsq_mvcc_scan_lock:
//   K23b k_mm_scan_flags: one lane per lock of the range — start_ts <= max_ts; tsq_launch_scan64 -> the rank of every hit
//   K23c k_mm_scan_place: start_ts and lock index at the rank, key and primary lengths; tsq_launch_scan64 x 2 -> the offsets
//        (the host reads the count and the two byte sizes once)
//        k_mw_copy x 2  : the keys' and the primaries' cells, compacted
// tsq_mvcc_resolve_lock:
//   K23d k_mm_resolve   : one lane per lock of the range — a binary search of the sorted transaction list, on a hit the drop of the lock
//                         and the add record (type, start_ts, commit_ts, value source) at its place in the key's chain (binary search)
//        tsq_mw_apply over the records; their key bytes are the store's own lock-key cells
// tsq_mvcc_gc:
//   K23e k_mm_gc_locks  : one lane per lock of the range — start_ts <= safe_point: an atomic count and atomicMin of the index
//   K23f k_mm_gc_keys   : one lane per key of the range — lo by a binary search over the chain, the keeper by a walk; chains of the
//                         threshold length or more by the whole wave in 64-entry steps
//        (the host reads the lock count: with one, nothing is written)
//   K23g k_mm_gc_mark   : one lane per ENTRY of the range — p >= lo[ord[p]] && p != keeper[ord[p]]: its drop mark; the drops counted
//        tsq_mw_apply over the marks
// tsq_mvcc_delete_range:
//   K23h k_mm_mark_range: the drop marks of entries [e0, e1) and locks [l0, l1); tsq_mw_apply over the marks
#include "tsq_mvcc_store.h"
#include "tsq_mvcc_maint_dp.h"

#include <algorithm>
#include <vector>

#define TSQ_MM_DEFAULT_WAVE_CHAIN 64  // TSQ_KNOB_MVCC_WAVE_CHAIN, as the reads and the writes
#define TSQ_MM_E_INTERNAL 0x8000u     // an ordinal outside the range's keys

struct MmCtl {
    MwCtl w;  // (first: the apply's words)
    tsq_mm_bounds b;
    int64_t k0, k1;  // the keys with versions of the range, ordinals [k0, k1)
    unsigned long long drops;
};

struct MmArgs {
    tsq_mw_store st;
    const int32_t* ord;  // [n] the ordinal of every entry among the K keys with versions
    const int32_t* seg;  // [K + 1]
    int64_t K;
    const int64_t* lpoff;
    const uint8_t* rng;  // start, then end
    int64_t slen, elen;
    MmCtl* ctl;
    tsq_mm_bounds b;  // (after the host's read)
    int64_t k0, nk;
    uint64_t ts;  // max_ts / safe_point
    int64_t chain_wave;
    // ScanLock
    int64_t* rank;    // [cnt + 1]
    int32_t* didx;    // [cnt]
    int64_t* okoff;   // [cnt + 1]
    int64_t* opoff;   // [cnt + 1]
    uint64_t* ostart; // [cnt]
    int64_t* oidx;    // [cnt]
    // ResolveLock: the list, and the records of the apply
    const uint64_t* txn_start;
    const uint64_t* txn_commit;
    int64_t T;
    uint8_t* flags;
    uint8_t* vtype;
    int32_t* vsrc;
    int32_t* vpos;
    int32_t* lpos;
    int64_t* rank_av;
    int64_t* rank_rv;
    int64_t* rank_al;
    int64_t* rank_dl;
    uint64_t* rec_sts;
    uint64_t* rec_cts;
    // GC
    int32_t* glo;    // [nk]
    int32_t* gkeep;  // [nk]
    // the marks
    int64_t* vw;
    uint8_t* vdrop;
    int64_t* lw;
    uint8_t* ldrop;
};

__global__ void __launch_bounds__(64) k_mm_bounds(MmArgs a) {
    if (threadIdx.x != 0 || blockIdx.x != 0) return;
    tsq_mm_bounds b;
    tsq_mm_range(a.st, a.rng, a.slen, a.rng + a.slen, a.elen, &b);
    a.ctl->b = b;
    // (e0 and e1 are first entries of keys or n: the keys with versions in between are ordinals [ord[e0], ord[e1]))
    a.ctl->k0 = b.e0 < a.st.n ? (int64_t)a.ord[b.e0] : a.K;
    a.ctl->k1 = b.e1 < a.st.n ? (int64_t)a.ord[b.e1] : a.K;
}

__global__ void __launch_bounds__(256) k_mm_scan_flags(MmArgs a) {
    const int64_t cnt = a.b.l1 - a.b.l0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x)
        a.rank[i] = tsq_mm_lock_le(a.st.s.l_start, a.b.l0 + i, a.ts) ? 1 : 0;
}
// (after the scan: rank[i + 1] - rank[i] is the flag, rank[cnt] the total <= cnt; the output arrays have cnt slots)
__global__ void __launch_bounds__(256) k_mm_scan_place(MmArgs a) {
    const int64_t cnt = a.b.l1 - a.b.l0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t d = a.rank[i];
        const bool hit = a.rank[i + 1] != d && d >= 0 && d < cnt;
        a.didx[i] = hit ? (int32_t)d : -1;
        if (hit) {
            const int64_t j = a.b.l0 + i;
            a.ostart[d] = a.st.s.l_start[j];
            a.oidx[d] = j;
            a.okoff[d] = a.st.lkoff[j + 1] - a.st.lkoff[j];
            a.opoff[d] = a.lpoff[j + 1] - a.lpoff[j];
        }
    }
}

__global__ void __launch_bounds__(256) k_mm_resolve(MmArgs a) {
    const int64_t cnt = a.b.l1 - a.b.l0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < cnt; i += (int64_t)gridDim.x * blockDim.x) {
        const int64_t j = a.b.l0 + i;
        tsq_mw_plan o;
        tsq_mm_resolve(a.st, j, a.txn_start, a.txn_commit, a.T, &o);
        a.flags[i] = o.flags;
        a.vtype[i] = o.vtype;
        a.vsrc[i] = o.vsrc;
        a.vpos[i] = o.vpos;
        a.lpos[i] = o.lpos;
        a.rank_av[i] = (o.flags & TSQ_MW_ADD_VERSION) ? 1 : 0;
        a.rank_rv[i] = (o.flags & TSQ_MW_REP_VERSION) ? 1 : 0;
        a.rank_al[i] = 0;
        a.rank_dl[i] = (o.flags & TSQ_MW_DROP_LOCK) ? 1 : 0;
        a.rec_sts[i] = a.st.s.l_start[j];
        a.rec_cts[i] = o.vcts;
    }
}

__global__ void __launch_bounds__(256) k_mm_gc_locks(MmArgs a) {
    const int lane = threadIdx.x & 63;
    unsigned long long nerr = 0, first = ~0ull;
    for (int64_t j = a.b.l0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.b.l1; j += (int64_t)gridDim.x * blockDim.x) {
        if (tsq_mm_lock_le(a.st.s.l_start, j, a.ts)) {
            nerr++;
            if ((unsigned long long)j < first) first = (unsigned long long)j;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        nerr += __shfl_xor(nerr, o, 64);
        const unsigned long long f = __shfl_xor(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        if (nerr) atomicAdd(&a.ctl->w.n_errors, nerr);
        if (first != ~0ull) atomicMin(&a.ctl->w.first_error, first);
    }
}

__global__ void __launch_bounds__(256) k_mm_gc_keys(MmArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t i0 = wave * 64; i0 < a.nk; i0 += nwaves * 64) {  // (wave uniform)
        const int64_t i = i0 + lane;
        const bool in = i < a.nk;
        int64_t lo = 0, e = 0, first = -1;
        bool by_wave = false;
        if (in) {
            const int64_t k = a.k0 + i;  // (k0 + nk <= K: seg has K + 1 entries)
            const int64_t s = a.seg[k];
            e = a.seg[k + 1];
            lo = tsq_mm_gc_lo(a.st.s.cts, s, e, a.ts);
            by_wave = a.chain_wave > 0 && e - s >= a.chain_wave;
            if (!by_wave) first = tsq_mm_gc_first(a.st.s.types, lo, e);
        }
        unsigned long long todo = __ballot(by_wave);
        while (todo) {  // (wave uniform)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t wlo = (int64_t)__shfl((unsigned long long)lo, src, 64), we = (int64_t)__shfl((unsigned long long)e, src, 64);
            int64_t f = -1;
            for (int64_t j0 = wlo; j0 < we; j0 += 64) {  // (wave uniform)
                const unsigned long long bal = __ballot(tsq_mv_decides(a.st.s.types, j0 + lane, we));
                if (bal) {
                    f = j0 + (__ffsll((long long)bal) - 1);
                    break;
                }
            }
            if (lane == src) first = f;
        }
        if (in) {
            a.glo[i] = (int32_t)lo;
            a.gkeep[i] = (int32_t)tsq_mm_gc_keeper(a.st.s.types, first);
        }
    }
}

// one lane per entry of [e0, e1): a coalesced stream; the key's two indices through the entry's ordinal
__global__ void __launch_bounds__(256) k_mm_gc_mark(MmArgs a) {
    const int lane = threadIdx.x & 63;
    unsigned long long drops = 0;
    unsigned int err = 0;
    for (int64_t p = a.b.e0 + (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.b.e1; p += (int64_t)gridDim.x * blockDim.x) {
        const int64_t k = (int64_t)a.ord[p] - a.k0;
        if (k < 0 || k >= a.nk) {
            err |= TSQ_MM_E_INTERNAL;
            continue;
        }
        if (tsq_mm_gc_drops(p, a.glo[k], a.gkeep[k])) {
            a.vdrop[p] = 1;
            a.vw[p + 1] = -1;
            drops++;
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        drops += __shfl_xor(drops, o, 64);
        err |= __shfl_xor(err, o, 64);
    }
    if (lane == 0) {
        if (drops) atomicAdd(&a.ctl->drops, drops);
        if (err) atomicOr(&a.ctl->w.err, err);
    }
}

__global__ void __launch_bounds__(256) k_mm_mark_range(MmArgs a) {
    const int64_t ne = a.b.e1 - a.b.e0, nl = a.b.l1 - a.b.l0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < ne + nl; i += (int64_t)gridDim.x * blockDim.x) {
        if (i < ne) {
            a.vdrop[a.b.e0 + i] = 1;
            a.vw[a.b.e0 + i + 1] = -1;
        } else {
            a.ldrop[a.b.l0 + (i - ne)] = 1;
            a.lw[a.b.l0 + (i - ne) + 1] = -1;
        }
    }
}

// ====================================================================== host side
namespace {
// what every range call holds: the range on the device, the control words, the bounds
struct MmCall {
    DevBuf rng, ctlb;
    MmArgs a;
    MmCtl ctl;
    float ms = 0;  // the device time of the bound and mark passes
};

tsq_status mm_interval(tsq_mvcc* m, MmCall* c) {  // ev[0] .. ev[1], both recorded and reached
    float ms = 0;
    if (hipEventElapsedTime(&ms, m->ev[0], m->ev[1]) == hipSuccess) c->ms += ms;
    return TSQ_OK;
}

// the checks every call shares, the range to the device, K23a and the host's read of the bounds
tsq_status mm_begin(tsq_mvcc* m, const char* what, bool writable, const uint8_t* start, int64_t slen, const uint8_t* end, int64_t elen, MmCall* c) {
    tsq_handle_hdr* h = &m->hdr;
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (slen < 0 || elen < 0 || (slen > 0 && !start) || (elen > 0 && !end)) return tsq_fail(h, TSQ_ERR_INVALID, std::string(what) + ": bad range");
    if (writable && !m->rw)
        return tsq_fail(h, TSQ_ERR_INVALID, std::string(what) + ": the store was created without start_ts and lock values (tsq_mvcc_create_rw)");
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    TSQ_TRY(tsq_mv_copy_in(ctx, h, c->rng, start, (size_t)slen, false, 0, (size_t)(slen + elen)));
    TSQ_TRY(tsq_mv_copy_in(ctx, h, c->rng, end, (size_t)elen, false, (size_t)slen, (size_t)(slen + elen)));
    TSQ_TRY(c->ctlb.reserve(ctx, h, sizeof(MmCtl) + 64));
    MmArgs& a = c->a;
    memset(&a, 0, sizeof a);
    tsq_mv_store_view(m, &a.st.s);
    a.st.sts = m->sts.as<uint64_t>();
    a.st.n = m->n;
    a.st.lkeys = m->keys.as<uint8_t>() + m->key_bytes;
    a.st.lkoff = m->lkoff.as<int64_t>();
    a.st.n_locks = m->n_locks;
    a.ord = m->ord.as<int32_t>();
    a.seg = m->seg.as<int32_t>();
    a.K = m->K;
    a.lpoff = m->lpoff.as<int64_t>();
    a.rng = c->rng.as<uint8_t>();
    a.slen = slen, a.elen = elen;
    a.ctl = c->ctlb.as<MmCtl>();
    a.chain_wave = tsq_knob(ctx, TSQ_KNOB_MVCC_WAVE_CHAIN, TSQ_MM_DEFAULT_WAVE_CHAIN);
    memset(&c->ctl, 0, sizeof c->ctl);
    c->ctl.w.first_error = ~0ull;
    TSQ_HIP(h, hipMemcpyAsync(a.ctl, &c->ctl, sizeof c->ctl, hipMemcpyHostToDevice, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // (the source is the caller's object: the copy has left it)
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_mm_bounds, dim3(1), dim3(64), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&c->ctl, a.ctl, sizeof c->ctl, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    mm_interval(m, c);
    const tsq_mm_bounds& b = c->ctl.b;
    if (b.u0 < 0 || b.u1 < b.u0 || b.u1 > m->U || b.e0 < 0 || b.e1 < b.e0 || b.e1 > m->n || b.l0 < 0 || b.l1 < b.l0 || b.l1 > m->n_locks || c->ctl.k0 < 0 ||
        c->ctl.k1 < c->ctl.k0 || c->ctl.k1 > m->K)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the bounds of the mvcc range are out of range");
    a.b = b;
    a.k0 = c->ctl.k0;
    a.nk = c->ctl.k1 - c->ctl.k0;
    return TSQ_OK;
}

void mm_result_zero(tsq_mvcc_maint_result* r) {
    memset(r, 0, sizeof *r);
    r->first_error = -1;
}

// the apply over the caller's marks alone (GC, DeleteRange): no records
tsq_status mm_apply_marks(tsq_mvcc* m, MmCall* c, tsq_mw_marks* marks, int64_t vdrops, int64_t ldrops, tsq_mvcc_maint_result* result, tsq_mvcc** next) {
    tsq_handle_hdr* h = &m->hdr;
    tsq_ctx* ctx = m->ctx;
    DevBuf ranks;
    StreamDrain drain(ctx->stream);
    TSQ_TRY(ranks.reserve(ctx, h, 4 * 8 + 64));
    TSQ_HIP(h, hipMemsetAsync(ranks.p, 0, 4 * 8, ctx->stream));
    tsq_mw_apply_in in;
    memset(&in, 0, sizeof in);
    in.rank_av = ranks.as<int64_t>(), in.rank_rv = ranks.as<int64_t>() + 1, in.rank_al = ranks.as<int64_t>() + 2, in.rank_dl = ranks.as<int64_t>() + 3;
    in.marks = marks;
    in.pre_vdrops = vdrops, in.pre_ldrops = ldrops;
    in.null_when_unchanged = true;
    in.ctl = &c->a.ctl->w;
    tsq_mw_apply_out out;
    TSQ_TRY(tsq_mw_apply(m, in, &out, next));
    result->versions_removed = vdrops;
    result->locks_removed = ldrops;
    result->mark_ms = c->ms;
    result->kernel_ms = c->ms + out.ms;
    return TSQ_OK;
}
}  // namespace

TSQ_API tsq_status tsq_mvcc_scan_lock(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len, uint64_t max_ts,
                                      tsq_mvcc_lock_scan* result) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (result) memset(result, 0, sizeof *result);
    m->sl_n = -1;
    if (!result) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_scan_lock: NULL argument");
    MmCall c;
    DevBuf rank, didx, scan_tmp;
    tsq_ctx* ctx = m->ctx;
    StreamDrain drain(ctx->stream);
    TSQ_TRY(mm_begin(m, "tsq_mvcc_scan_lock", false, start, start_len, end, end_len, &c));
    MmArgs& a = c.a;
    const int64_t cnt = a.b.l1 - a.b.l0;
    if (cnt == 0) {
        m->sl_n = 0, m->sl_key_bytes = m->sl_prim_bytes = 0;
        result->kernel_ms = c.ms;
        return TSQ_OK;
    }
    TSQ_TRY(rank.reserve(ctx, h, ((size_t)cnt + 1) * 8 + 64));
    TSQ_TRY(didx.reserve(ctx, h, (size_t)cnt * 4 + 64));
    TSQ_TRY(m->sl_koff.reserve(ctx, h, ((size_t)cnt + 1) * 8 + 64));
    TSQ_TRY(m->sl_poff.reserve(ctx, h, ((size_t)cnt + 1) * 8 + 64));
    TSQ_TRY(m->sl_start.reserve(ctx, h, (size_t)cnt * 8 + 64));
    TSQ_TRY(m->sl_idx.reserve(ctx, h, (size_t)cnt * 8 + 64));
    a.ts = max_ts;
    a.rank = rank.as<int64_t>();
    a.didx = didx.as<int32_t>();
    a.okoff = m->sl_koff.as<int64_t>();
    a.opoff = m->sl_poff.as<int64_t>();
    a.ostart = m->sl_start.as<uint64_t>();
    a.oidx = m->sl_idx.as<int64_t>();
    // (the lengths of the slots no hit reaches are zero: the offsets behind the last hit all equal the byte total)
    TSQ_HIP(h, hipMemsetAsync(a.okoff, 0, ((size_t)cnt + 1) * 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(a.opoff, 0, ((size_t)cnt + 1) * 8, ctx->stream));
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    const int grid = tsq_grid_for(ctx, cnt, 256);
    hipLaunchKernelGGL(k_mm_scan_flags, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.rank, cnt, scan_tmp));
    hipLaunchKernelGGL(k_mm_scan_place, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.okoff, cnt, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, a.opoff, cnt, scan_tmp));
    int64_t tot[3] = {0, 0, 0};
    TSQ_HIP(h, hipMemcpyAsync(&tot[0], a.rank + cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&tot[1], a.okoff + cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&tot[2], a.opoff + cnt, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (tot[0] < 0 || tot[0] > cnt || tot[1] < 0 || tot[1] > m->lkey_bytes || tot[2] < 0 || tot[2] > m->lprim_bytes)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the counts of the mvcc lock scan are out of range");
    TSQ_TRY(m->sl_keys.reserve(ctx, h, (size_t)tot[1] + 64));
    TSQ_TRY(m->sl_prim.reserve(ctx, h, (size_t)tot[2] + 64));
    TSQ_TRY(tsq_mw_copy(ctx, h, a.st.lkeys, a.st.lkoff + a.b.l0, nullptr, false, m->sl_keys.as<uint8_t>(), a.okoff, a.didx, cnt));
    TSQ_TRY(tsq_mw_copy(ctx, h, m->lprim.as<uint8_t>(), a.lpoff + a.b.l0, nullptr, false, m->sl_prim.as<uint8_t>(), a.opoff, a.didx, cnt));
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    mm_interval(m, &c);
    m->sl_n = tot[0], m->sl_key_bytes = tot[1], m->sl_prim_bytes = tot[2];
    result->n_locks = tot[0];
    result->key_bytes = tot[1];
    result->primary_bytes = tot[2];
    result->kernel_ms = c.ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_scan_lock_fetch(tsq_mvcc* m, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* primaries, int64_t primary_cap,
                                            int64_t* primary_offsets, uint64_t* start_ts, int64_t* lock_index, uint32_t flags) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (m->sl_n < 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_scan_lock_fetch: no successful lock scan to fetch");
    const int64_t n = m->sl_n;
    if (!key_offsets || !primary_offsets || key_cap < 0 || primary_cap < 0 || (n > 0 && (!start_ts || !lock_index)))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_scan_lock_fetch: bad arguments");
    if (key_cap < m->sl_key_bytes || primary_cap < m->sl_prim_bytes || (m->sl_key_bytes > 0 && !keys) || (m->sl_prim_bytes > 0 && !primaries))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_scan_lock_fetch: output buffer too small");
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const hipMemcpyKind kind = (flags & TSQ_COL_DEVICE) ? hipMemcpyDeviceToDevice : hipMemcpyDeviceToHost;
    if (n == 0) {
        static const int64_t zero = 0;
        TSQ_HIP(h, hipMemcpyAsync(key_offsets, &zero, 8, (flags & TSQ_COL_DEVICE) ? hipMemcpyHostToDevice : hipMemcpyHostToHost, ctx->stream));
        TSQ_HIP(h, hipMemcpyAsync(primary_offsets, &zero, 8, (flags & TSQ_COL_DEVICE) ? hipMemcpyHostToDevice : hipMemcpyHostToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        return TSQ_OK;
    }
    const struct {
        void* dst;
        const void* src;
        size_t bytes;
    } parts[] = {{keys, m->sl_keys.p, (size_t)m->sl_key_bytes},     {key_offsets, m->sl_koff.p, ((size_t)n + 1) * 8},
                 {primaries, m->sl_prim.p, (size_t)m->sl_prim_bytes}, {primary_offsets, m->sl_poff.p, ((size_t)n + 1) * 8},
                 {start_ts, m->sl_start.p, (size_t)n * 8},          {lock_index, m->sl_idx.p, (size_t)n * 8}};
    for (const auto& p : parts)
        if (p.bytes) TSQ_HIP(h, hipMemcpyAsync(p.dst, p.src, p.bytes, kind, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_resolve_lock(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len, const uint64_t* txn_start_ts,
                                         const uint64_t* txn_commit_ts, int64_t n_txns, tsq_mvcc_maint_result* result, tsq_mvcc** next) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (next) *next = nullptr;
    if (result) mm_result_zero(result);
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (!result || !next || n_txns < 0 || (n_txns > 0 && (!txn_start_ts || !txn_commit_ts))) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_resolve_lock: bad arguments");
    if (!m->rw) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_resolve_lock: the store was created without start_ts and lock values (tsq_mvcc_create_rw)");
    // (every lock of the range may add a version)
    if (n_txns >= (1LL << 31) || m->n + 2 * m->n_locks >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "mvcc resolve lock: 2^31 entries or more");
    std::vector<std::pair<uint64_t, uint64_t>> txns((size_t)n_txns);
    for (int64_t i = 0; i < n_txns; i++) txns[(size_t)i] = {txn_start_ts[i], txn_commit_ts[i]};
    std::sort(txns.begin(), txns.end());
    for (int64_t i = 0; i < n_txns; i++) {
        const auto& t = txns[(size_t)i];
        if (i > 0 && txns[(size_t)i - 1].first == t.first) return tsq_fail(h, TSQ_ERR_INVALID, "mvcc resolve lock: a start_ts given twice");
        if (t.second == UINT64_MAX || (t.second == 0 && t.first == UINT64_MAX))
            return tsq_fail(h, TSQ_ERR_INVALID, "mvcc resolve lock: commitTS 2^64 - 1 is the lock's version");
    }
    MmCall c;
    DevBuf tl, flags, vtype, vsrc, vpos, lpos, rank_av, rank_rv, rank_al, rank_dl, rec_sts, rec_cts, av, al, vdst_new, ldst_new;
    tsq_mw_marks marks;
    tsq_ctx* ctx = m->ctx;
    StreamDrain drain(ctx->stream);
    TSQ_TRY(mm_begin(m, "tsq_mvcc_resolve_lock", true, start, start_len, end, end_len, &c));
    MmArgs& a = c.a;
    const int64_t q = a.b.l1 - a.b.l0, T = n_txns;
    if (q == 0 || T == 0) {
        result->mark_ms = result->kernel_ms = c.ms;
        return TSQ_OK;
    }
    std::vector<uint64_t> flat((size_t)T * 2);
    for (int64_t i = 0; i < T; i++) flat[(size_t)i] = txns[(size_t)i].first, flat[(size_t)(T + i)] = txns[(size_t)i].second;
    TSQ_TRY(tsq_mv_copy_in(ctx, h, tl, flat.data(), (size_t)T * 16, false));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // (flat is a local)
    TSQ_TRY(flags.reserve(ctx, h, (size_t)q + 64));
    TSQ_TRY(vtype.reserve(ctx, h, (size_t)q + 64));
    for (DevBuf* b : {&vsrc, &vpos, &lpos, &vdst_new, &ldst_new, &av, &al}) TSQ_TRY(b->reserve(ctx, h, (size_t)q * 4 + 64));
    for (DevBuf* b : {&rank_av, &rank_rv, &rank_al, &rank_dl}) TSQ_TRY(b->reserve(ctx, h, ((size_t)q + 1) * 8 + 64));
    for (DevBuf* b : {&rec_sts, &rec_cts}) TSQ_TRY(b->reserve(ctx, h, (size_t)q * 8 + 64));
    a.txn_start = tl.as<uint64_t>();
    a.txn_commit = tl.as<uint64_t>() + T;
    a.T = T;
    a.flags = flags.as<uint8_t>();
    a.vtype = vtype.as<uint8_t>();
    a.vsrc = vsrc.as<int32_t>();
    a.vpos = vpos.as<int32_t>();
    a.lpos = lpos.as<int32_t>();
    a.rank_av = rank_av.as<int64_t>();
    a.rank_rv = rank_rv.as<int64_t>();
    a.rank_al = rank_al.as<int64_t>();
    a.rank_dl = rank_dl.as<int64_t>();
    a.rec_sts = rec_sts.as<uint64_t>();
    a.rec_cts = rec_cts.as<uint64_t>();
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_mm_resolve, dim3(tsq_grid_for(ctx, q, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    mm_interval(m, &c);
    TSQ_TRY(tsq_mw_marks_init(m, h, &marks));
    tsq_mw_apply_in in;
    memset(&in, 0, sizeof in);
    in.q = q;
    in.rkeys = a.st.lkeys;
    in.rkoff = a.st.lkoff + a.b.l0;
    in.rkey_bytes = m->lkey_bytes;
    in.flags = a.flags, in.vtype = a.vtype, in.vsrc = a.vsrc, in.vpos = a.vpos, in.lpos = a.lpos;
    in.rank_av = a.rank_av, in.rank_rv = a.rank_rv, in.rank_al = a.rank_al, in.rank_dl = a.rank_dl;
    in.av = av.as<int32_t>(), in.al = al.as<int32_t>(), in.vdst_new = vdst_new.as<int32_t>(), in.ldst_new = ldst_new.as<int32_t>();
    in.rec_sts = a.rec_sts, in.rec_cts = a.rec_cts;
    in.values_from_locks = true;
    in.marks = &marks;
    in.null_when_unchanged = true;
    in.ctl = &a.ctl->w;
    tsq_mw_apply_out out;
    TSQ_TRY(tsq_mw_apply(m, in, &out, next));
    result->versions_added = out.addv;
    result->versions_replaced = out.repv;
    result->locks_removed = out.dropl;
    result->mark_ms = c.ms;
    result->kernel_ms = c.ms + out.ms;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_gc(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len, uint64_t safe_point,
                               tsq_mvcc_maint_result* result, tsq_mvcc** next) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (next) *next = nullptr;
    if (result) mm_result_zero(result);
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (!result || !next) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_gc: NULL argument");
    MmCall c;
    DevBuf glo, gkeep;
    tsq_mw_marks marks;
    tsq_ctx* ctx = m->ctx;
    StreamDrain drain(ctx->stream);
    TSQ_TRY(mm_begin(m, "tsq_mvcc_gc", true, start, start_len, end, end_len, &c));
    MmArgs& a = c.a;
    a.ts = safe_point;
    const int64_t nlk = a.b.l1 - a.b.l0, ne = a.b.e1 - a.b.e0;
    TSQ_TRY(glo.reserve(ctx, h, (size_t)a.nk * 4 + 64));
    TSQ_TRY(gkeep.reserve(ctx, h, (size_t)a.nk * 4 + 64));
    a.glo = glo.as<int32_t>();
    a.gkeep = gkeep.as<int32_t>();
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    if (nlk > 0) hipLaunchKernelGGL(k_mm_gc_locks, dim3(tsq_grid_for(ctx, nlk, 256)), dim3(256), 0, ctx->stream, a);
    if (a.nk > 0) hipLaunchKernelGGL(k_mm_gc_keys, dim3(tsq_grid_for(ctx, a.nk, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&c.ctl, a.ctl, sizeof c.ctl, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    mm_interval(m, &c);
    const int64_t nerr = (int64_t)c.ctl.w.n_errors;
    if (nerr < 0 || nerr > nlk || (nerr > 0 && (c.ctl.w.first_error < (unsigned long long)a.b.l0 || c.ctl.w.first_error >= (unsigned long long)a.b.l1)))
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the lock count of the mvcc gc is out of range");
    result->mark_ms = result->kernel_ms = c.ms;
    if (nerr > 0) {  // (:1041-1047) nothing is written
        result->n_errors = nerr;
        result->first_error = (int64_t)c.ctl.w.first_error;
        return TSQ_OK;
    }
    if (ne == 0) return TSQ_OK;
    TSQ_TRY(tsq_mw_marks_init(m, h, &marks));
    a.vw = marks.vw.as<int64_t>();
    a.vdrop = marks.vdrop.as<uint8_t>();
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_mm_gc_mark, dim3(tsq_grid_for(ctx, ne, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&c.ctl, a.ctl, sizeof c.ctl, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    mm_interval(m, &c);
    result->mark_ms = result->kernel_ms = c.ms;
    if (c.ctl.w.err) return tsq_fail(h, TSQ_ERR_HIP, "internal: an ordinal of the mvcc gc leaves the range's keys");
    const int64_t drops = (int64_t)c.ctl.drops;
    if (drops < 0 || drops > ne) return tsq_fail(h, TSQ_ERR_HIP, "internal: the drop count of the mvcc gc is out of range");
    if (drops == 0) return TSQ_OK;
    return mm_apply_marks(m, &c, &marks, drops, 0, result, next);
}

TSQ_API tsq_status tsq_mvcc_delete_range(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len,
                                         tsq_mvcc_maint_result* result, tsq_mvcc** next) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (next) *next = nullptr;
    if (result) mm_result_zero(result);
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (!result || !next) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_delete_range: NULL argument");
    MmCall c;
    tsq_mw_marks marks;
    tsq_ctx* ctx = m->ctx;
    StreamDrain drain(ctx->stream);
    TSQ_TRY(mm_begin(m, "tsq_mvcc_delete_range", true, start, start_len, end, end_len, &c));
    result->mark_ms = result->kernel_ms = c.ms;
    // the reference's bounds are EncodeBytes(start) and EncodeBytes(end) as raw LevelDB keys (:1088-1090): no key sorts under
    // EncodeBytes("") — an empty end deletes nothing
    if (end_len == 0) return TSQ_OK;
    MmArgs& a = c.a;
    const int64_t ne = a.b.e1 - a.b.e0, nlk = a.b.l1 - a.b.l0;
    if (ne + nlk == 0) return TSQ_OK;
    TSQ_TRY(tsq_mw_marks_init(m, h, &marks));
    a.vw = marks.vw.as<int64_t>();
    a.vdrop = marks.vdrop.as<uint8_t>();
    a.lw = marks.lw.as<int64_t>();
    a.ldrop = marks.ldrop.as<uint8_t>();
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    hipLaunchKernelGGL(k_mm_mark_range, dim3(tsq_grid_for(ctx, ne + nlk, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    mm_interval(m, &c);
    return mm_apply_marks(m, &c, &marks, ne, nlk, result, next);
}
