// tsq_mvcc_write.hip — the MVCC writes on the GPU (gfx950): Prewrite, Commit and Rollback of the reference's MVCCLevelDB
// (store/mockstore/mocktikv/mvcc_leveldb.go:442-717) applied to a tsq_mvcc store in HBM, into the NEXT store — a new handle; the
// store a write was called on stays as it is (include/tsq.h "MVCC writes").  The per-key code is tsq_mvcc_write_dp.h.
//
// one write call:
//   K22a k_mw_verdict   : one lane per request key — the key against its left neighbour (order, offsets, op, the empty put), its
//                         lower bound in the key universe and the equality test, the lock, the head of the chain or (Commit,
//                         Rollback) the walk for start_ts == startTS — chains of the threshold length or more by the whole wave in
//                         64-version steps — the insertion index inside the chain and whether an equal version goes; the flags of
//                         the four request-side ranks; the error count and atomicMin of the first error
//        (the host reads the control words and the verdicts; the apply runs only when no verdict is an error)
//        tsq_launch_scan64 x 4: new versions / replaced versions / new locks / dropped locks before every request key
//   K22b k_mw_adders / k_mw_mark: one lane per request key — the insertion indices by rank, then the length of every run of equal
//                         indices at its insertion point (two adds per run), -1 behind the replaced versions and the dropped locks,
//                         their drop flags
//        tsq_launch_scan64 x 2 over n + 1 and n_locks + 1: every surviving old entry moves to old index + insertions at or before
//        it - drops before it; a new one goes to insertion index + new ones before it - drops before it
//   K22c k_mw_place_versions / K22d k_mw_place_locks / K22e k_mw_place_new: the fixed-width fields at their new index, key / value /
//                         primary lengths into the new offset arrays; tsq_launch_scan64 over each turns them into the offsets
//        (the host reads the byte totals, which size the next store's byte buffers)
//   K22f k_mw_copy      : the bytes of one family of cells (old keys, old values, request keys, ...) to their new place; a cell of
//                         64 bytes or more is copied by the whole wave, as k_rg_copy does
//   then the create kernels of tsq_mvcc.hip over the new arrays (tsq_mv_index): their checks are the internal assertion
//   (everything behind the verdicts is tsq_mw_apply, which the range calls of tsq_mvcc_maint.hip feed with their own marks and records)
// tsq_mvcc_create_rw: K22g k_mw_lockvals — one lane per lock: its value's offsets, the put lock with an empty value
#include "tsq_mvcc_store.h"
#include "tsq_mvcc_write_dp.h"

#define TSQ_MW_DEFAULT_WAVE_CHAIN 64  // TSQ_KNOB_MVCC_WAVE_CHAIN, as the reads
#define TSQ_MW_WAVE_COPY 64
#define TSQ_MW_E_INTERNAL 0x8000u     // a new index outside the next store

struct MwArgs {
    tsq_mw_store st;
    tsq_mw_req r;
    int64_t chain_wave;
    MwCtl* ctl;
    // the plan, per request key
    uint8_t* verdict;
    uint64_t* info;  // [2 q]
    uint8_t* flags;
    uint8_t* vtype;
    int32_t* vsrc;
    int32_t* vpos;
    int32_t* lpos;
    int64_t* rank_av;  // [q + 1] each: the flag, then (scan) the count before the key
    int64_t* rank_rv;
    int64_t* rank_al;
    int64_t* rank_dl;
};

__global__ void __launch_bounds__(256) k_mw_verdict(MwArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    unsigned int ebits = 0;
    unsigned long long nerr = 0, first = ~0ull;
    for (int64_t i0 = wave * 64; i0 < a.r.q; i0 += nwaves * 64) {  // (wave uniform)
        const int64_t i = i0 + lane;
        const bool in = i < a.r.q;
        bool valid = false, by_wave = false;
        tsq_mw_place p;
        p.u = 0, p.eq = false, p.lock = -1, p.s = p.e = 0;
        int64_t found = -1;
        if (in) {
            const uint32_t e = tsq_mw_req_check(a.r, i);
            ebits |= e;
            valid = e == 0;
            if (valid) {
                const int64_t kb = a.r.koff[i];
                tsq_mw_locate(a.st, a.r.keys + kb, a.r.koff[i + 1] - kb, &p);
                const bool walk = tsq_mw_needs_walk(a.st, a.r, p);
                by_wave = walk && a.chain_wave > 0 && p.e - p.s >= a.chain_wave;
                if (walk && !by_wave) found = tsq_mw_find_start(a.st.sts, p.s, p.e, a.r.start_ts);
            }
        }
        unsigned long long todo = __ballot(by_wave);
        while (todo) {  // (wave uniform)
            const int src = __ffsll((long long)todo) - 1;
            todo &= todo - 1;
            const int64_t ws = (int64_t)__shfl((unsigned long long)p.s, src, 64), we = (int64_t)__shfl((unsigned long long)p.e, src, 64);
            int64_t f = -1;
            for (int64_t j0 = ws; j0 < we; j0 += 64) {  // (wave uniform)
                const unsigned long long bal = __ballot(tsq_mw_is_start(a.st.sts, j0 + lane, we, a.r.start_ts));
                if (bal) {
                    f = j0 + (__ffsll((long long)bal) - 1);
                    break;
                }
            }
            if (lane == src) found = f;
        }
        if (in) {
            tsq_mw_plan o;
            tsq_mw_plan_none(&o);
            if (valid) tsq_mw_decide(a.st, a.r, i, p, found, &o);
            a.verdict[i] = o.verdict;
            a.info[2 * i] = o.info0;
            a.info[2 * i + 1] = o.info1;
            a.flags[i] = o.flags;
            a.vtype[i] = o.vtype;
            a.vsrc[i] = o.vsrc;
            a.vpos[i] = o.vpos;
            a.lpos[i] = o.lpos;
            a.rank_av[i] = (o.flags & TSQ_MW_ADD_VERSION) ? 1 : 0;
            a.rank_rv[i] = (o.flags & TSQ_MW_REP_VERSION) ? 1 : 0;
            a.rank_al[i] = (o.flags & TSQ_MW_ADD_LOCK) ? 1 : 0;
            a.rank_dl[i] = (o.flags & TSQ_MW_DROP_LOCK) ? 1 : 0;
            if (o.verdict >= TSQ_MVCC_V_LOCKED) {
                nerr++;
                if ((unsigned long long)i < first) first = (unsigned long long)i;
            }
        }
    }
    for (int o = 32; o > 0; o >>= 1) {
        ebits |= __shfl_xor(ebits, o, 64);
        nerr += __shfl_xor(nerr, o, 64);
        const unsigned long long f = __shfl_xor(first, o, 64);
        first = f < first ? f : first;
    }
    if (lane == 0) {
        if (ebits) atomicOr(&a.ctl->err, ebits);
        if (nerr) atomicAdd(&a.ctl->n_errors, nerr);
        if (first != ~0ull) atomicMin(&a.ctl->first_error, first);
    }
}

struct MwApplyArgs {
    // the current store
    const int64_t* koff;
    const uint64_t* cts;
    const uint64_t* sts;
    const uint8_t* types;
    const int64_t* voff;
    int64_t n;
    const int64_t* lkoff;
    const uint64_t* lstart;
    const uint64_t* lttl;
    const uint8_t* lops;
    const int64_t* lpoff;
    const int64_t* lvoff;
    int64_t nl;
    // the marks: vw [n + 2], lw [nl + 2] (k_mw_mark adds the records' to the caller's, then they are scanned), vdrop [n], ldrop [nl]
    int64_t* vw;
    uint8_t* vdrop;
    int64_t* lw;
    uint8_t* ldrop;
    // the records and their plan
    int64_t q;
    const int64_t* rkoff;
    const int64_t* rvoff;  // prewrite
    const uint8_t* rops;   // prewrite
    const uint8_t* flags;
    const uint8_t* vtype;
    const int32_t* vsrc;
    const int32_t* vpos;
    const int32_t* lpos;
    const int64_t* rank_av;
    const int64_t* rank_rv;
    const int64_t* rank_al;
    const int64_t* rank_dl;
    int32_t* av;  // [q]: the version index of the a-th record that adds a version (a = its rank), al likewise for the locks
    int32_t* al;
    const uint64_t* rec_sts;  // [q] or NULL: start_ts / new_cts for every record
    const uint64_t* rec_cts;
    uint64_t start_ts, new_cts, ttl;
    int64_t primary_len;
    // the next store
    int64_t n2, nl2;
    uint64_t* cts2;
    uint64_t* sts2;
    uint8_t* types2;
    int64_t* koff2;  // lengths, then (scan) offsets
    int64_t* voff2;
    uint64_t* lstart2;
    uint64_t* lttl2;
    uint8_t* lops2;
    int64_t* lkoff2;
    int64_t* lpoff2;
    int64_t* lvoff2;
    // where every cell goes (-1: nowhere)
    int32_t* vdst_old;  // [n]
    int32_t* ldst_old;  // [nl]
    int32_t* vdst_new;  // [q]
    int32_t* ldst_new;  // [q]
    MwCtl* ctl;
};

// the insertion indices of the keys that add a version (a lock), by their rank: the request is sorted, so equal indices are a run
__global__ void __launch_bounds__(256) k_mw_adders(MwApplyArgs a) {
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.q; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t f = a.flags[i];
        if (f & TSQ_MW_ADD_VERSION) a.av[a.rank_av[i]] = a.vpos[i];  // (ranks < their totals <= q)
        if (f & TSQ_MW_ADD_LOCK) a.al[a.rank_al[i]] = a.lpos[i];
    }
}
// The length of a run of r adders at one index goes into w[index] as -(rank of its first) + (rank of its last + 1): two adds per
// index however long the run — a transaction that appends behind the last key is ONE run (one add per key on one word measured
// 4.5 x the whole apply at 2^22 keys).
__device__ __forceinline__ void mw_mark_run(int64_t* w, const int32_t* idx, int64_t rank, int64_t total, int64_t at) {
    if (rank == 0 || idx[rank - 1] != (int32_t)at) atomicAdd((unsigned long long*)&w[at], (unsigned long long)(-rank));
    if (rank == total - 1 || idx[rank + 1] != (int32_t)at) atomicAdd((unsigned long long*)&w[at], (unsigned long long)(rank + 1));
}
// (only after a request without errors: vpos <= n, a replaced vpos < n, lpos <= n_locks, a dropped lpos < n_locks — the plan's
// indices come from searches bounded by the store's counts; checked again here)
__global__ void __launch_bounds__(256) k_mw_mark(MwApplyArgs a) {
    unsigned int e = 0;
    const int64_t n_av = a.rank_av[a.q], n_al = a.rank_al[a.q];
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.q; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t f = a.flags[i];
        const int64_t vp = a.vpos[i], lp = a.lpos[i];
        if (f & TSQ_MW_ADD_VERSION) {
            if (vp < 0 || vp > a.n || ((f & TSQ_MW_REP_VERSION) && vp >= a.n)) {
                e |= TSQ_MW_E_INTERNAL;
            } else {
                mw_mark_run(a.vw, a.av, a.rank_av[i], n_av, vp);
                if (f & TSQ_MW_REP_VERSION) {
                    atomicAdd((unsigned long long*)&a.vw[vp + 1], ~0ull);
                    a.vdrop[vp] = 1;
                }
            }
        }
        if (f & (TSQ_MW_ADD_LOCK | TSQ_MW_DROP_LOCK)) {
            if (lp < 0 || lp > a.nl || ((f & TSQ_MW_DROP_LOCK) && lp >= a.nl)) {
                e |= TSQ_MW_E_INTERNAL;
            } else {
                if (f & TSQ_MW_ADD_LOCK) mw_mark_run(a.lw, a.al, a.rank_al[i], n_al, lp);
                if (f & TSQ_MW_DROP_LOCK) {
                    atomicAdd((unsigned long long*)&a.lw[lp + 1], ~0ull);
                    a.ldrop[lp] = 1;
                }
            }
        }
    }
    if (e) atomicOr(&a.ctl->err, e);
}

__global__ void __launch_bounds__(256) k_mw_place_versions(MwApplyArgs a) {
    unsigned int e = 0;
    for (int64_t p = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; p < a.n; p += (int64_t)gridDim.x * blockDim.x) {
        int64_t d = a.vdrop[p] ? -1 : p + a.vw[p + 1];
        if (d >= a.n2 || (!a.vdrop[p] && d < 0)) {
            e |= TSQ_MW_E_INTERNAL;
            d = -1;
        }
        a.vdst_old[p] = (int32_t)d;
        if (d >= 0) {
            a.cts2[d] = a.cts[p];
            a.sts2[d] = a.sts[p];
            a.types2[d] = a.types[p];
            a.koff2[d] = a.koff[p + 1] - a.koff[p];
            a.voff2[d] = a.voff[p + 1] - a.voff[p];
        }
    }
    if (e) atomicOr(&a.ctl->err, e);
}
__global__ void __launch_bounds__(256) k_mw_place_locks(MwApplyArgs a) {
    unsigned int e = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < a.nl; j += (int64_t)gridDim.x * blockDim.x) {
        int64_t d = a.ldrop[j] ? -1 : j + a.lw[j + 1];
        if (d >= a.nl2 || (!a.ldrop[j] && d < 0)) {
            e |= TSQ_MW_E_INTERNAL;
            d = -1;
        }
        a.ldst_old[j] = (int32_t)d;
        if (d >= 0) {
            a.lstart2[d] = a.lstart[j];
            a.lttl2[d] = a.lttl[j];
            a.lops2[d] = a.lops[j];
            a.lkoff2[d] = a.lkoff[j + 1] - a.lkoff[j];
            a.lpoff2[d] = a.lpoff[j + 1] - a.lpoff[j];
            a.lvoff2[d] = a.lvoff[j + 1] - a.lvoff[j];
        }
    }
    if (e) atomicOr(&a.ctl->err, e);
}
__global__ void __launch_bounds__(256) k_mw_place_new(MwApplyArgs a) {
    unsigned int e = 0;
    for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.q; i += (int64_t)gridDim.x * blockDim.x) {
        const uint8_t f = a.flags[i];
        const int64_t klen = a.rkoff[i + 1] - a.rkoff[i];
        int64_t vd = -1, ld = -1;
        if (f & TSQ_MW_ADD_VERSION) {
            vd = (int64_t)a.vpos[i] + a.rank_av[i] - a.rank_rv[i];
            const int32_t j = a.vsrc[i];
            if (vd < 0 || vd >= a.n2 || j >= a.nl) {
                e |= TSQ_MW_E_INTERNAL;
                vd = -1;
            } else {
                a.cts2[vd] = a.rec_cts ? a.rec_cts[i] : a.new_cts;
                a.sts2[vd] = a.rec_sts ? a.rec_sts[i] : a.start_ts;
                a.types2[vd] = a.vtype[i];
                a.koff2[vd] = klen;
                a.voff2[vd] = j >= 0 ? a.lvoff[j + 1] - a.lvoff[j] : 0;
            }
        }
        if (f & TSQ_MW_ADD_LOCK) {
            ld = (int64_t)a.lpos[i] + a.rank_al[i] - a.rank_dl[i];
            if (ld < 0 || ld >= a.nl2) {
                e |= TSQ_MW_E_INTERNAL;
                ld = -1;
            } else {
                a.lstart2[ld] = a.start_ts;
                a.lttl2[ld] = a.ttl;
                a.lops2[ld] = a.rops[i];
                a.lkoff2[ld] = klen;
                a.lpoff2[ld] = a.primary_len;
                a.lvoff2[ld] = a.rvoff[i + 1] - a.rvoff[i];
            }
        }
        a.vdst_new[i] = (int32_t)vd;
        a.ldst_new[i] = (int32_t)ld;
    }
    if (e) atomicOr(&a.ctl->err, e);
}

// cell r of one family goes to cell didx[r] of the next store (-1: nowhere); its bytes come from cell sidx[r] of the source (NULL: cell
// r; single: cell 0).  The length is the destination's; a cell without bytes reads no source index.
struct MwCopyArgs {
    const uint8_t* src;
    const int64_t* soff;
    const int32_t* sidx;
    int32_t single;
    uint8_t* dst;
    const int64_t* doff;
    const int32_t* didx;
    int64_t cnt;
};
__global__ void __launch_bounds__(256) k_mw_copy(MwCopyArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t wave = ((int64_t)blockIdx.x * blockDim.x + threadIdx.x) >> 6, nwaves = ((int64_t)gridDim.x * blockDim.x) >> 6;
    for (int64_t r0 = wave * 64; r0 < a.cnt; r0 += nwaves * 64) {  // (wave uniform)
        const int64_t r = r0 + lane;
        const int64_t di = r < a.cnt ? a.didx[r] : -1;
        int64_t len = 0;
        const uint8_t* s = a.src;
        uint8_t* d = a.dst;
        if (di >= 0) {
            const int64_t o0 = a.doff[di];
            len = a.doff[di + 1] - o0;
            d = a.dst + o0;
            if (len > 0) s = a.src + a.soff[a.single ? 0 : (a.sidx ? (int64_t)a.sidx[r] : r)];
        }
        const bool by_wave = len >= TSQ_MW_WAVE_COPY;
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

__global__ void __launch_bounds__(256) k_mw_lockvals(const int64_t* lvoff, int64_t lval_bytes, const uint8_t* lops, int64_t nl, unsigned int* err) {
    unsigned int e = 0;
    for (int64_t j = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; j < nl; j += (int64_t)gridDim.x * blockDim.x) {
        if (!tsq_mv_pair_ok(lvoff, j, lval_bytes)) e |= TSQ_MV_E_OFFSETS;
        else if (lops[j] == TSQ_MVCC_OP_PUT && lvoff[j + 1] == lvoff[j]) e |= TSQ_MV_E_EMPTY_PUT;
    }
    if (e) atomicOr(err, e);
}

// ====================================================================== host side
namespace {
const char* mw_request_message(unsigned int e) {
    if (e & TSQ_MW_E_OFFSETS) return "mvcc write: offsets decrease or leave their buffer";
    if (e & TSQ_MW_E_EMPTY_KEY) return "mvcc write: empty key";
    if (e & TSQ_MW_E_OP) return "mvcc write: a prewrite op other than Put, Del or Lock";
    if (e & TSQ_MW_E_EMPTY_PUT) return "mvcc write: a put with an empty value";
    return "mvcc write: keys not strictly ascending";
}

tsq_status mw_write(tsq_mvcc* m, int kind, const tsq_mvcc_write_req* req, uint8_t* verdicts, uint64_t* info, tsq_mvcc_write_result* result, tsq_mvcc** next) {
    tsq_handle_hdr* h = &m->hdr;
    if (next) *next = nullptr;
    if (result) memset(result, 0, sizeof *result);
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (!req || !result || !next) return tsq_fail(h, TSQ_ERR_INVALID, "mvcc write: NULL argument");
    result->first_error = -1;
    if (!m->rw) return tsq_fail(h, TSQ_ERR_INVALID, "mvcc write: the store was created without start_ts and lock values (tsq_mvcc_create_rw)");
    const int64_t q = req->n_keys, n = m->n, nl = m->n_locks;
    if (q < 0 || req->key_bytes < 0 || req->value_bytes < 0 || req->primary_len < 0) return tsq_fail(h, TSQ_ERR_INVALID, "mvcc write: negative count");
    if (q >= (1LL << 31) || n + nl + q >= (1LL << 31)) return tsq_fail(h, TSQ_ERR_UNSUPPORTED, "mvcc write: 2^31 entries or more");
    if ((kind == TSQ_MW_COMMIT && req->commit_ts == UINT64_MAX) || (kind == TSQ_MW_ROLLBACK && req->start_ts == UINT64_MAX))
        return tsq_fail(h, TSQ_ERR_INVALID, "mvcc write: commitTS 2^64 - 1 is the lock's version");
    const bool pre = kind == TSQ_MW_PREWRITE;
    if ((q > 0 && !req->key_offsets) || (req->key_bytes > 0 && !req->keys) || (pre && q > 0 && (!req->ops || !req->value_offsets)) ||
        (pre && req->value_bytes > 0 && !req->values) || (pre && req->primary_len > 0 && !req->primary))
        return tsq_fail(h, TSQ_ERR_INVALID, "mvcc write: NULL array");
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const bool dev = req->flags & TSQ_COL_DEVICE;

    // every temporary of the call; the drain behind them waits for the kernels that use them on every exit
    DevBuf rkeys, rkoff, rops, rvals, rvoff, prim, ctlb, verdict, infob, flags, vtype, vsrc, vpos, lpos, rank_av, rank_rv, rank_al, rank_dl, vdst_new, ldst_new, av,
        al;
    tsq_mw_marks marks;
    StreamDrain drain(ctx->stream);

    // the request on the device
    const uint8_t* d_keys = req->keys;
    const int64_t* d_koff = req->key_offsets;
    const uint8_t* d_ops = req->ops;
    const uint8_t* d_vals = req->values;
    const int64_t* d_voff = req->value_offsets;
    static const int64_t zero_off = 0;
    if (!dev || q == 0) {
        TSQ_TRY(tsq_mv_copy_in(ctx, h, rkeys, req->keys, q ? (size_t)req->key_bytes : 0, false));
        TSQ_TRY(tsq_mv_copy_in(ctx, h, rkoff, q ? (const void*)req->key_offsets : &zero_off, ((size_t)q + 1) * 8, false));
        d_keys = rkeys.as<uint8_t>();
        d_koff = rkoff.as<int64_t>();
        if (pre) {
            TSQ_TRY(tsq_mv_copy_in(ctx, h, rops, req->ops, (size_t)q, false));
            TSQ_TRY(tsq_mv_copy_in(ctx, h, rvals, req->values, q ? (size_t)req->value_bytes : 0, false));
            TSQ_TRY(tsq_mv_copy_in(ctx, h, rvoff, q ? (const void*)req->value_offsets : &zero_off, ((size_t)q + 1) * 8, false));
            d_ops = rops.as<uint8_t>();
            d_vals = rvals.as<uint8_t>();
            d_voff = rvoff.as<int64_t>();
        }
    }
    const int64_t prim_off[2] = {0, pre ? req->primary_len : 0};  // the primary as a family of one cell: its bytes behind its two offsets
    if (pre) {
        TSQ_TRY(tsq_mv_copy_in(ctx, h, prim, prim_off, 16, false, 0, 16 + (size_t)req->primary_len));
        TSQ_TRY(tsq_mv_copy_in(ctx, h, prim, req->primary, (size_t)req->primary_len, false, 16, 16 + (size_t)req->primary_len));
    }

    MwArgs a;
    memset(&a, 0, sizeof a);
    tsq_mv_store_view(m, &a.st.s);
    a.st.sts = m->sts.as<uint64_t>();
    a.st.n = n;
    a.st.lkeys = m->keys.as<uint8_t>() + m->key_bytes;
    a.st.lkoff = m->lkoff.as<int64_t>();
    a.st.n_locks = nl;
    a.r.keys = d_keys;
    a.r.koff = d_koff;
    a.r.key_bytes = q ? req->key_bytes : 0;
    a.r.q = q;
    a.r.ops = d_ops;
    a.r.voff = d_voff;
    a.r.value_bytes = q ? req->value_bytes : 0;
    a.r.kind = kind;
    a.r.start_ts = req->start_ts;
    a.r.commit_ts = req->commit_ts;
    a.chain_wave = tsq_knob(ctx, TSQ_KNOB_MVCC_WAVE_CHAIN, TSQ_MW_DEFAULT_WAVE_CHAIN);
    TSQ_TRY(ctlb.reserve(ctx, h, sizeof(MwCtl) + 64));
    TSQ_TRY(verdict.reserve(ctx, h, (size_t)q + 64));
    TSQ_TRY(infob.reserve(ctx, h, (size_t)q * 16 + 64));
    TSQ_TRY(flags.reserve(ctx, h, (size_t)q + 64));
    TSQ_TRY(vtype.reserve(ctx, h, (size_t)q + 64));
    for (DevBuf* b : {&vsrc, &vpos, &lpos, &vdst_new, &ldst_new, &av, &al}) TSQ_TRY(b->reserve(ctx, h, (size_t)q * 4 + 64));
    for (DevBuf* b : {&rank_av, &rank_rv, &rank_al, &rank_dl}) TSQ_TRY(b->reserve(ctx, h, ((size_t)q + 1) * 8 + 64));
    a.ctl = ctlb.as<MwCtl>();
    a.verdict = verdict.as<uint8_t>();
    a.info = infob.as<uint64_t>();
    a.flags = flags.as<uint8_t>();
    a.vtype = vtype.as<uint8_t>();
    a.vsrc = vsrc.as<int32_t>();
    a.vpos = vpos.as<int32_t>();
    a.lpos = lpos.as<int32_t>();
    a.rank_av = rank_av.as<int64_t>();
    a.rank_rv = rank_rv.as<int64_t>();
    a.rank_al = rank_al.as<int64_t>();
    a.rank_dl = rank_dl.as<int64_t>();

    float ms = 0;
    MwCtl ctl;
    memset(&ctl, 0, sizeof ctl);
    ctl.first_error = ~0ull;
    TSQ_HIP(h, hipMemcpyAsync(a.ctl, &ctl, sizeof ctl, hipMemcpyHostToDevice, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));  // (ctl is a local: the copy has left it)
    TSQ_HIP(h, hipEventRecord(m->ev[0], ctx->stream));
    if (q > 0) hipLaunchKernelGGL(k_mw_verdict, dim3(tsq_grid_for(ctx, q, 256)), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(m->ev[1], ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&ctl, a.ctl, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (hipEventElapsedTime(&ms, m->ev[0], m->ev[1]) == hipSuccess) result->kernel_ms += ms;
    if (ctl.err) return tsq_fail(h, TSQ_ERR_INVALID, mw_request_message(ctl.err));
    if ((int64_t)ctl.n_errors < 0 || (int64_t)ctl.n_errors > q || (ctl.n_errors > 0 && ctl.first_error >= (unsigned long long)q))
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the error count of the mvcc write is out of range");
    if (verdicts && q > 0) TSQ_HIP(h, hipMemcpyAsync(verdicts, a.verdict, (size_t)q, hipMemcpyDeviceToHost, ctx->stream));
    if (info && q > 0) TSQ_HIP(h, hipMemcpyAsync(info, a.info, (size_t)q * 16, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    result->n_errors = (int64_t)ctl.n_errors;
    result->first_error = ctl.n_errors ? (int64_t)ctl.first_error : -1;
    if (ctl.n_errors) return TSQ_OK;  // nothing is written

    // ---- the apply
    TSQ_TRY(tsq_mw_marks_init(m, h, &marks));
    tsq_mw_apply_in in;
    memset(&in, 0, sizeof in);
    in.q = q;
    in.rkeys = d_keys, in.rkoff = d_koff, in.rkey_bytes = a.r.key_bytes;
    in.flags = a.flags, in.vtype = a.vtype, in.vsrc = a.vsrc, in.vpos = a.vpos, in.lpos = a.lpos;
    in.rank_av = a.rank_av, in.rank_rv = a.rank_rv, in.rank_al = a.rank_al, in.rank_dl = a.rank_dl;
    in.av = av.as<int32_t>(), in.al = al.as<int32_t>(), in.vdst_new = vdst_new.as<int32_t>(), in.ldst_new = ldst_new.as<int32_t>();
    in.start_ts = req->start_ts;
    in.new_cts = kind == TSQ_MW_COMMIT ? req->commit_ts : req->start_ts;
    in.ttl = req->ttl;
    in.values_from_locks = kind == TSQ_MW_COMMIT;
    in.rops = d_ops, in.rvals = d_vals, in.rvoff = d_voff, in.rvalue_bytes = a.r.value_bytes;
    if (pre) in.prim = prim.as<uint8_t>() + 16, in.prim_off = prim.as<int64_t>();
    in.primary_len = pre ? req->primary_len : 0;
    in.marks = &marks;
    in.ctl = a.ctl;
    tsq_mw_apply_out out;
    TSQ_TRY(tsq_mw_apply(m, in, &out, next));
    result->kernel_ms += out.ms;
    result->versions_added = out.addv;
    result->versions_replaced = out.repv;
    result->locks_added = out.addl;
    result->locks_removed = out.dropl;
    return TSQ_OK;
}
}  // namespace

tsq_status tsq_mw_copy(tsq_ctx* ctx, tsq_handle_hdr* h, const uint8_t* src, const int64_t* soff, const int32_t* sidx, bool single, uint8_t* dst, const int64_t* doff,
                       const int32_t* didx, int64_t cnt) {
    if (cnt <= 0) return TSQ_OK;
    MwCopyArgs c;
    c.src = src, c.soff = soff, c.sidx = sidx, c.single = single ? 1 : 0, c.dst = dst, c.doff = doff, c.didx = didx, c.cnt = cnt;
    hipLaunchKernelGGL(k_mw_copy, dim3(tsq_grid_for(ctx, cnt, 256)), dim3(256), 0, ctx->stream, c);
    TSQ_HIP(h, hipGetLastError());
    return TSQ_OK;
}


tsq_status tsq_mw_marks_init(tsq_mvcc* m, tsq_handle_hdr* h, tsq_mw_marks* k) {
    tsq_ctx* ctx = m->ctx;
    const size_t n = (size_t)m->n, nl = (size_t)m->n_locks;
    TSQ_TRY(k->vw.reserve(ctx, h, (n + 2) * 8 + 64));
    TSQ_TRY(k->vdrop.reserve(ctx, h, n + 64));
    TSQ_TRY(k->lw.reserve(ctx, h, (nl + 2) * 8 + 64));
    TSQ_TRY(k->ldrop.reserve(ctx, h, nl + 64));
    TSQ_HIP(h, hipMemsetAsync(k->vw.p, 0, (n + 2) * 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(k->vdrop.p, 0, n + 1, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(k->lw.p, 0, (nl + 2) * 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(k->ldrop.p, 0, nl + 1, ctx->stream));
    return TSQ_OK;
}

tsq_status tsq_mw_apply(tsq_mvcc* m, const tsq_mw_apply_in& in, tsq_mw_apply_out* out, tsq_mvcc** next) {
    tsq_handle_hdr* h = &m->hdr;
    tsq_ctx* ctx = m->ctx;
    const int64_t q = in.q, n = m->n, nl = m->n_locks;
    memset(out, 0, sizeof *out);
    *next = nullptr;
    if (in.pre_vdrops < 0 || in.pre_vdrops > n || in.pre_ldrops < 0 || in.pre_ldrops > nl)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the counts of the mvcc write are out of range");
    DevBuf vdst_old, ldst_old, scan_tmp;
    std::unique_ptr<tsq_mvcc> nx;
    StreamDrain drain(ctx->stream);  // every exit waits for the kernels that use them
    float ms = 0;
    MwCtl ctl;
    memset(&ctl, 0, sizeof ctl);
    TSQ_HIP(h, hipEventRecord(m->ev[2], ctx->stream));
    TSQ_TRY(tsq_launch_scan64(ctx, h, in.rank_av, q, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, in.rank_rv, q, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, in.rank_al, q, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, in.rank_dl, q, scan_tmp));
    int64_t tot[4] = {0, 0, 0, 0};
    TSQ_HIP(h, hipMemcpyAsync(&tot[0], in.rank_av + q, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&tot[1], in.rank_rv + q, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&tot[2], in.rank_al + q, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&tot[3], in.rank_dl + q, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t addv = tot[0], repv = tot[1], addl = tot[2], dropl = tot[3];
    if (addv < 0 || addv > q || repv < 0 || repv > addv || repv + in.pre_vdrops > n || addl < 0 || addl > q || dropl < 0 || dropl > q || dropl + in.pre_ldrops > nl)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the counts of the mvcc write are out of range");
    out->addv = addv, out->repv = repv, out->addl = addl, out->dropl = dropl;
    if (in.null_when_unchanged && addv + addl + dropl + in.pre_vdrops + in.pre_ldrops == 0) return TSQ_OK;
    const int64_t n2 = n + addv - repv - in.pre_vdrops, nl2 = nl + addl - dropl - in.pre_ldrops;

    TSQ_TRY(tsq_mv_new(ctx, h, &nx));
    nx->rw = true;
    nx->n = n2;
    nx->n_locks = nl2;
    TSQ_TRY(vdst_old.reserve(ctx, h, (size_t)n * 4 + 64));
    TSQ_TRY(ldst_old.reserve(ctx, h, (size_t)nl * 4 + 64));

    // the next store's fixed-width arrays and offsets (the lengths first; zeroed, so that a slot no entry reaches holds no bytes)
    TSQ_TRY(nx->cts.reserve(ctx, h, (size_t)n2 * 8 + 64));
    TSQ_TRY(nx->sts.reserve(ctx, h, (size_t)n2 * 8 + 64));
    TSQ_TRY(nx->types.reserve(ctx, h, (size_t)n2 + 64));
    TSQ_TRY(nx->koff.reserve(ctx, h, ((size_t)n2 + 1) * 8 + 64));
    TSQ_TRY(nx->voff.reserve(ctx, h, ((size_t)n2 + 1) * 8 + 64));
    TSQ_TRY(nx->lstart.reserve(ctx, h, (size_t)nl2 * 8 + 64));
    TSQ_TRY(nx->lttl.reserve(ctx, h, (size_t)nl2 * 8 + 64));
    TSQ_TRY(nx->lops.reserve(ctx, h, (size_t)nl2 + 64));
    for (DevBuf* b : {&nx->lkoff, &nx->lpoff, &nx->lvoff}) TSQ_TRY(b->reserve(ctx, h, ((size_t)nl2 + 1) * 8 + 64));
    for (DevBuf* b : {&nx->koff, &nx->voff}) TSQ_HIP(h, hipMemsetAsync(b->p, 0, ((size_t)n2 + 1) * 8, ctx->stream));
    for (DevBuf* b : {&nx->lkoff, &nx->lpoff, &nx->lvoff}) TSQ_HIP(h, hipMemsetAsync(b->p, 0, ((size_t)nl2 + 1) * 8, ctx->stream));
    MwApplyArgs p;
    memset(&p, 0, sizeof p);
    p.koff = m->koff.as<int64_t>();
    p.cts = m->cts.as<uint64_t>();
    p.sts = m->sts.as<uint64_t>();
    p.types = m->types.as<uint8_t>();
    p.voff = m->voff.as<int64_t>();
    p.n = n;
    p.lkoff = m->lkoff.as<int64_t>();
    p.lstart = m->lstart.as<uint64_t>();
    p.lttl = m->lttl.as<uint64_t>();
    p.lops = m->lops.as<uint8_t>();
    p.lpoff = m->lpoff.as<int64_t>();
    p.lvoff = m->lvoff.as<int64_t>();
    p.nl = nl;
    p.vw = in.marks->vw.as<int64_t>(), p.vdrop = in.marks->vdrop.as<uint8_t>(), p.lw = in.marks->lw.as<int64_t>(), p.ldrop = in.marks->ldrop.as<uint8_t>();
    p.q = q;
    p.rkoff = in.rkoff;
    p.rvoff = in.rvoff;
    p.rops = in.rops;
    p.flags = in.flags, p.vtype = in.vtype, p.vsrc = in.vsrc, p.vpos = in.vpos, p.lpos = in.lpos;
    p.rank_av = in.rank_av, p.rank_rv = in.rank_rv, p.rank_al = in.rank_al, p.rank_dl = in.rank_dl;
    p.av = in.av, p.al = in.al;
    p.rec_sts = in.rec_sts, p.rec_cts = in.rec_cts;
    p.start_ts = in.start_ts;
    p.new_cts = in.new_cts;
    p.ttl = in.ttl;
    p.primary_len = in.primary_len;
    p.n2 = n2, p.nl2 = nl2;
    p.cts2 = nx->cts.as<uint64_t>();
    p.sts2 = nx->sts.as<uint64_t>();
    p.types2 = nx->types.as<uint8_t>();
    p.koff2 = nx->koff.as<int64_t>();
    p.voff2 = nx->voff.as<int64_t>();
    p.lstart2 = nx->lstart.as<uint64_t>();
    p.lttl2 = nx->lttl.as<uint64_t>();
    p.lops2 = nx->lops.as<uint8_t>();
    p.lkoff2 = nx->lkoff.as<int64_t>();
    p.lpoff2 = nx->lpoff.as<int64_t>();
    p.lvoff2 = nx->lvoff.as<int64_t>();
    p.vdst_old = vdst_old.as<int32_t>();
    p.ldst_old = ldst_old.as<int32_t>();
    p.vdst_new = in.vdst_new;
    p.ldst_new = in.ldst_new;
    p.ctl = in.ctl;
    if (q > 0) hipLaunchKernelGGL(k_mw_adders, dim3(tsq_grid_for(ctx, q, 256)), dim3(256), 0, ctx->stream, p);
    if (q > 0) hipLaunchKernelGGL(k_mw_mark, dim3(tsq_grid_for(ctx, q, 256)), dim3(256), 0, ctx->stream, p);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, p.vw, n + 1, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, p.lw, nl + 1, scan_tmp));
    if (n > 0) hipLaunchKernelGGL(k_mw_place_versions, dim3(tsq_grid_for(ctx, n, 256)), dim3(256), 0, ctx->stream, p);
    if (nl > 0) hipLaunchKernelGGL(k_mw_place_locks, dim3(tsq_grid_for(ctx, nl, 256)), dim3(256), 0, ctx->stream, p);
    if (q > 0) hipLaunchKernelGGL(k_mw_place_new, dim3(tsq_grid_for(ctx, q, 256)), dim3(256), 0, ctx->stream, p);
    TSQ_HIP(h, hipGetLastError());
    TSQ_TRY(tsq_launch_scan64(ctx, h, p.koff2, n2, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, p.voff2, n2, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, p.lkoff2, nl2, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, p.lpoff2, nl2, scan_tmp));
    TSQ_TRY(tsq_launch_scan64(ctx, h, p.lvoff2, nl2, scan_tmp));
    int64_t by[5] = {0, 0, 0, 0, 0};
    TSQ_HIP(h, hipMemcpyAsync(&by[0], p.koff2 + n2, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&by[1], p.voff2 + n2, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&by[2], p.lkoff2 + nl2, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&by[3], p.lpoff2 + nl2, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&by[4], p.lvoff2 + nl2, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&ctl, in.ctl, sizeof ctl, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (ctl.err) return tsq_fail(h, TSQ_ERR_HIP, "internal: a new index of the mvcc write leaves the next store");
    const int64_t rkb = in.rkey_bytes, rvb = in.rvalue_bytes;
    if (by[0] < 0 || by[0] > m->key_bytes + rkb || by[1] < 0 || by[1] > m->value_bytes + m->lval_bytes || by[2] < 0 || by[2] > m->lkey_bytes + rkb || by[3] < 0 ||
        by[3] > m->lprim_bytes + q * p.primary_len || by[4] < 0 || by[4] > m->lval_bytes + rvb)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the byte counts of the mvcc write are out of range");
    nx->key_bytes = by[0];
    nx->value_bytes = by[1];
    nx->lkey_bytes = by[2];
    nx->lprim_bytes = by[3];
    nx->lval_bytes = by[4];
    TSQ_TRY(nx->keys.reserve(ctx, h, (size_t)(by[0] + by[2]) + 64));
    TSQ_TRY(nx->vals.reserve(ctx, h, (size_t)by[1] + 64));
    TSQ_TRY(nx->lprim.reserve(ctx, h, (size_t)by[3] + 64));
    TSQ_TRY(nx->lvals.reserve(ctx, h, (size_t)by[4] + 64));
    uint8_t* nkeys = nx->keys.as<uint8_t>();
    const uint8_t* lkeys = m->keys.as<uint8_t>() + m->key_bytes;
    // the old entries, then the new ones
    TSQ_TRY(tsq_mw_copy(ctx, h, m->keys.as<uint8_t>(), p.koff, nullptr, false, nkeys, p.koff2, p.vdst_old, n));
    TSQ_TRY(tsq_mw_copy(ctx, h, m->vals.as<uint8_t>(), p.voff, nullptr, false, nx->vals.as<uint8_t>(), p.voff2, p.vdst_old, n));
    TSQ_TRY(tsq_mw_copy(ctx, h, lkeys, p.lkoff, nullptr, false, nkeys + by[0], p.lkoff2, p.ldst_old, nl));
    TSQ_TRY(tsq_mw_copy(ctx, h, m->lprim.as<uint8_t>(), p.lpoff, nullptr, false, nx->lprim.as<uint8_t>(), p.lpoff2, p.ldst_old, nl));
    TSQ_TRY(tsq_mw_copy(ctx, h, m->lvals.as<uint8_t>(), p.lvoff, nullptr, false, nx->lvals.as<uint8_t>(), p.lvoff2, p.ldst_old, nl));
    if (addv > 0) {
        TSQ_TRY(tsq_mw_copy(ctx, h, in.rkeys, in.rkoff, nullptr, false, nkeys, p.koff2, p.vdst_new, q));
        if (in.values_from_locks) TSQ_TRY(tsq_mw_copy(ctx, h, m->lvals.as<uint8_t>(), p.lvoff, p.vsrc, false, nx->vals.as<uint8_t>(), p.voff2, p.vdst_new, q));
    }
    if (addl > 0) {
        TSQ_TRY(tsq_mw_copy(ctx, h, in.rkeys, in.rkoff, nullptr, false, nkeys + by[0], p.lkoff2, p.ldst_new, q));
        TSQ_TRY(tsq_mw_copy(ctx, h, in.rvals, in.rvoff, nullptr, false, nx->lvals.as<uint8_t>(), p.lvoff2, p.ldst_new, q));
        TSQ_TRY(tsq_mw_copy(ctx, h, in.prim, in.prim_off, nullptr, true, nx->lprim.as<uint8_t>(), p.lpoff2, p.ldst_new, q));
    }
    // the head flags, ordinals and universe; the create checks are the assertion that the merge kept both orders
    TSQ_TRY(tsq_mv_index(nx.get(), h, true));
    TSQ_HIP(h, hipEventRecord(m->ev[3], ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    if (hipEventElapsedTime(&ms, m->ev[2], m->ev[3]) == hipSuccess) out->ms = ms;
    *next = nx.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_create_rw(tsq_ctx* ctx, const tsq_mvcc_data* d, const uint8_t* lock_values, const int64_t* lock_value_offsets, int64_t lock_value_bytes,
                                      tsq_mvcc** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || !out || !d) return tsq_fail(nullptr, TSQ_ERR_INVALID, "tsq_mvcc_create_rw: NULL argument");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (d->n > 0 && !d->start_ts) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_mvcc_create_rw: a writable store needs start_ts");
    if (lock_value_bytes < 0 || (d->n_locks > 0 && !lock_value_offsets) || (lock_value_bytes > 0 && !lock_values))
        return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_mvcc_create_rw: NULL array");
    tsq_mvcc* m = nullptr;
    TSQ_TRY(tsq_mvcc_create(ctx, d, &m));
    std::unique_ptr<tsq_mvcc, void (*)(tsq_mvcc*)> hold(m, tsq_mvcc_destroy);
    const bool dev = d->data_flags & TSQ_COL_DEVICE;
    const int64_t nl = d->n_locks;
    static const int64_t zero_off = 0;
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->sts, d->start_ts, (size_t)d->n * 8, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lvals, lock_values, (size_t)lock_value_bytes, dev));
    TSQ_TRY(tsq_mv_copy_in(ctx, ch, m->lvoff, nl ? (const void*)lock_value_offsets : &zero_off, ((size_t)nl + 1) * 8, nl ? dev : false));
    unsigned int* err = &m->ctl.as<MvCtl>()->err;  // (zero: the store passed the create checks)
    if (nl > 0) hipLaunchKernelGGL(k_mw_lockvals, dim3(tsq_grid_for(ctx, nl, 256)), dim3(256), 0, ctx->stream, m->lvoff.as<int64_t>(), lock_value_bytes, m->lops.as<uint8_t>(), nl, err);
    TSQ_HIP(ch, hipGetLastError());
    unsigned int e = 0;
    TSQ_HIP(ch, hipMemcpyAsync(&e, err, 4, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(ch, hipStreamSynchronize(ctx->stream));
    if (e & TSQ_MV_E_OFFSETS) return tsq_fail(ch, TSQ_ERR_INVALID, "mvcc store: offsets decrease or leave their buffer");
    if (e) return tsq_fail(ch, TSQ_ERR_INVALID, "mvcc store: a put lock with an empty value");
    m->rw = true;
    m->lval_bytes = lock_value_bytes;
    *out = hold.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_prewrite(tsq_mvcc* m, const tsq_mvcc_write_req* req, uint8_t* verdicts, uint64_t* info, tsq_mvcc_write_result* result, tsq_mvcc** next) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    return mw_write(m, TSQ_MW_PREWRITE, req, verdicts, info, result, next);
}
TSQ_API tsq_status tsq_mvcc_commit(tsq_mvcc* m, const tsq_mvcc_write_req* req, uint8_t* verdicts, uint64_t* info, tsq_mvcc_write_result* result, tsq_mvcc** next) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    return mw_write(m, TSQ_MW_COMMIT, req, verdicts, info, result, next);
}
TSQ_API tsq_status tsq_mvcc_rollback(tsq_mvcc* m, const tsq_mvcc_write_req* req, uint8_t* verdicts, uint64_t* info, tsq_mvcc_write_result* result, tsq_mvcc** next) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    return mw_write(m, TSQ_MW_ROLLBACK, req, verdicts, info, result, next);
}

TSQ_API tsq_status tsq_mvcc_lock_at(tsq_mvcc* m, int64_t j, uint8_t* key, int64_t key_cap, int64_t* key_len, uint8_t* primary, int64_t primary_cap,
                                    int64_t* primary_len, uint64_t* start_ts, uint64_t* ttl, int32_t* op) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (j < 0 || j >= m->n_locks) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_lock_at: no such lock");
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    int64_t ko[2] = {0, 0}, po[2] = {0, 0};
    uint64_t ls = 0, lt = 0;
    uint8_t lo = 0;
    TSQ_HIP(h, hipMemcpyAsync(ko, m->lkoff.as<int64_t>() + j, 16, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(po, m->lpoff.as<int64_t>() + j, 16, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&ls, m->lstart.as<uint64_t>() + j, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&lt, m->lttl.as<uint64_t>() + j, 8, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipMemcpyAsync(&lo, m->lops.as<uint8_t>() + j, 1, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    const int64_t kl = ko[1] - ko[0], pl = po[1] - po[0];
    if (ko[0] < 0 || kl < 0 || ko[1] > m->lkey_bytes || po[0] < 0 || pl < 0 || po[1] > m->lprim_bytes)
        return tsq_fail(h, TSQ_ERR_HIP, "internal: the lock of the mvcc store is out of range");
    if (key_len) *key_len = kl;
    if (primary_len) *primary_len = pl;
    if (start_ts) *start_ts = ls;
    if (ttl) *ttl = lt;
    if (op) *op = (int32_t)lo;
    if (key_cap < kl || primary_cap < pl || (kl > 0 && !key) || (pl > 0 && !primary))
        return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_lock_at: buffer too small (the lengths are filled in)");
    if (kl) TSQ_HIP(h, hipMemcpyAsync(key, m->keys.as<uint8_t>() + m->key_bytes + ko[0], (size_t)kl, hipMemcpyDeviceToHost, ctx->stream));
    if (pl) TSQ_HIP(h, hipMemcpyAsync(primary, m->lprim.as<uint8_t>() + po[0], (size_t)pl, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_sizes(tsq_mvcc* m, tsq_mvcc_store_sizes* out) {
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    if (!out) return tsq_fail(&m->hdr, TSQ_ERR_INVALID, "tsq_mvcc_sizes: NULL argument");
    out->n = m->n;
    out->n_locks = m->n_locks;
    out->key_bytes = m->key_bytes;
    out->value_bytes = m->value_bytes;
    out->lock_key_bytes = m->lkey_bytes;
    out->lock_primary_bytes = m->lprim_bytes;
    out->lock_value_bytes = m->lval_bytes;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_mvcc_export(tsq_mvcc* m, const tsq_mvcc_arrays* o) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(m, TSQ_MAGIC_MVCC));
    if (!m || m->hdr.magic != TSQ_MAGIC_MVCC) return TSQ_ERR_INVALID;
    tsq_handle_hdr* h = &m->hdr;
    if (m->cancelled.load()) return tsq_fail(h, TSQ_ERR_CANCELLED, "mvcc store cancelled");
    if (!o) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_export: NULL argument");
    if (!m->rw) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_mvcc_export: the store was created without start_ts and lock values (tsq_mvcc_create_rw)");
    tsq_ctx* ctx = m->ctx;
    TSQ_HIP(h, hipSetDevice(ctx->device));
    const size_t n = (size_t)m->n, nl = (size_t)m->n_locks;
    const struct {
        void* dst;
        const void* src;
        size_t bytes;
    } parts[] = {{o->keys, m->keys.p, (size_t)m->key_bytes},
                 {o->key_offsets, m->koff.p, (n + 1) * 8},
                 {o->commit_ts, m->cts.p, n * 8},
                 {o->start_ts, m->sts.p, n * 8},
                 {o->types, m->types.p, n},
                 {o->values, m->vals.p, (size_t)m->value_bytes},
                 {o->value_offsets, m->voff.p, (n + 1) * 8},
                 {o->lock_keys, m->keys.as<uint8_t>() + m->key_bytes, (size_t)m->lkey_bytes},
                 {o->lock_key_offsets, m->lkoff.p, (nl + 1) * 8},
                 {o->lock_start_ts, m->lstart.p, nl * 8},
                 {o->lock_ttl, m->lttl.p, nl * 8},
                 {o->lock_ops, m->lops.p, nl},
                 {o->lock_primaries, m->lprim.p, (size_t)m->lprim_bytes},
                 {o->lock_primary_offsets, m->lpoff.p, (nl + 1) * 8},
                 {o->lock_values, m->lvals.p, (size_t)m->lval_bytes},
                 {o->lock_value_offsets, m->lvoff.p, (nl + 1) * 8}};
    for (const auto& c : parts)
        if (c.dst && c.bytes) TSQ_HIP(h, hipMemcpyAsync(c.dst, c.src, c.bytes, hipMemcpyDeviceToDevice, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    return TSQ_OK;
}
