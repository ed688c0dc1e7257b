// tsq_mvcc_store.h — the handle of an MVCC store, shared by its units: tsq_mvcc.hip (create, the snapshot reads) and
// tsq_mvcc_write.hip (the writable create, Prewrite / Commit / Rollback into the next store, the export) and tsq_mvcc_maint.hip
// (ScanLock, ResolveLock, GC, DeleteRange).
#ifndef TSQ_MVCC_STORE_H
#define TSQ_MVCC_STORE_H

#include "tsq_stage.h"
#include "tsq_mvcc_dp.h"

#include <memory>

#define TSQ_MAGIC_MVCC 0x7473714du /* 'tsqM' */

// the words of one scan the kernels share and the host reads once at the end
struct MvCtl {
    unsigned long long first_locked;  // atomicMin of the locked positions; ~0: none
    unsigned long long walked;        // version entries read
    unsigned long long total;         // chosen entries of all positions
    int64_t n_pairs;                  // pairs the call reports
    int64_t n_fetch;                  // pairs tsq_mvcc_fetch writes (0 after ErrLocked)
    int64_t locked;
    int64_t lock_j;
    int64_t key_beg, key_len, prim_beg, prim_len;
    uint64_t l_start, l_ttl;
    int64_t l_op;
    unsigned int err;
    unsigned int pad;
};

struct tsq_mvcc {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    std::atomic<int> cancelled{0};
    int64_t n = 0, n_locks = 0, key_bytes = 0, value_bytes = 0, lkey_bytes = 0, lprim_bytes = 0, K = 0, U = 0;
    // the store (keys: the versions' keys, then at key_bytes the locks' keys)
    DevBuf keys, koff, cts, types, vals, voff, lkoff, lstart, lttl, lops, lprim, lpoff;
    DevBuf head, ord, seg, ubeg, ulen, useg, ucnt, ulock;
    // a writable store (tsq_mvcc_create_rw, or the next store of a write) keeps what a write needs beyond a read
    bool rw = false;
    int64_t lval_bytes = 0;
    DevBuf sts, lvals, lvoff;
    // one scan
    DevBuf rbytes, roffs, rflags, rlo, rbase, chosen, bbase, sel, selpos, klens, vlens, rcounts, scan_tmp, ctl;
    MvCtl last;  // the words of the last scan
    bool have_last = false;
    int64_t last_key_bytes = 0, last_value_bytes = 0;
    int64_t scans = 0, examined = 0, walked = 0, pairs = 0;
    double kernel_ms = 0;
    DevEvent ev[4];  // the bound pass, then the passes behind the host's read of the position count
    // the last tsq_mvcc_scan_lock (tsq_mvcc_maint.hip): the locks it found, compacted; sl_n < 0: none to fetch
    DevBuf sl_keys, sl_koff, sl_prim, sl_poff, sl_start, sl_idx;
    int64_t sl_n = -1, sl_key_bytes = 0, sl_prim_bytes = 0;
};

// ---- the apply of tsq_mvcc_write.hip, shared by the writes and by the range calls of tsq_mvcc_maint.hip
// the words of one write or range call
struct MwCtl {
    unsigned int err;
    unsigned int pad;
    unsigned long long n_errors;
    unsigned long long first_error;  // ~0: none
};
// Marks over the current store: vdrop[p] / ldrop[j] = 1 for an entry / a lock that goes, vw [n + 2] / lw [n_locks + 2] the shift of
// every old index (scanned by the apply).  tsq_mw_marks_init zeroes them; a caller that drops entries itself writes vdrop[p] = 1 with
// vw[p + 1] = -1 (ldrop[j] = 1 with lw[j + 1] = -1) — one writer per entry — and tells the apply how many.
struct tsq_mw_marks {
    DevBuf vw, vdrop, lw, ldrop;
};
tsq_status tsq_mw_marks_init(tsq_mvcc* m, tsq_handle_hdr* h, tsq_mw_marks* k);
// The add / drop records of one call, q of them, ascending by key (device arrays).  Record i may add a version at entry index vpos[i]
// (TSQ_MW_ADD_VERSION, with TSQ_MW_REP_VERSION the entry there goes), add a lock at lock index lpos[i] (TSQ_MW_ADD_LOCK, a prewrite
// only) and drop the lock at lpos[i] (TSQ_MW_DROP_LOCK).
struct tsq_mw_apply_in {
    int64_t q;
    const uint8_t* rkeys;  // the records' key cells: the request of a write, the store's lock-key cells of a resolve
    const int64_t* rkoff;  // [q + 1]
    int64_t rkey_bytes;
    const uint8_t* flags;
    const uint8_t* vtype;
    const int32_t* vsrc;  // the lock whose value becomes the new version's value, or -1: empty
    const int32_t* vpos;
    const int32_t* lpos;
    int64_t* rank_av;  // [q + 1] each: the flag of every record; scanned by the apply
    int64_t* rank_rv;
    int64_t* rank_al;
    int64_t* rank_dl;
    int32_t* av;  // [q] each: scratch of the apply
    int32_t* al;
    int32_t* vdst_new;
    int32_t* ldst_new;
    const uint64_t* rec_sts;  // [q] a new version's startTS and commitTS by record, or NULL: start_ts / new_cts for all
    const uint64_t* rec_cts;
    uint64_t start_ts, new_cts, ttl;
    bool values_from_locks;  // a new version carries the value of lock vsrc (a commit)
    // a prewrite's new locks
    const uint8_t* rops;
    const uint8_t* rvals;
    const int64_t* rvoff;
    int64_t rvalue_bytes;
    const uint8_t* prim;       // the primary as a family of one cell
    const int64_t* prim_off;   // [2]
    int64_t primary_len;
    tsq_mw_marks* marks;       // initialised; with the caller's own drops in them
    int64_t pre_vdrops, pre_ldrops;
    bool null_when_unchanged;  // nothing added and nothing dropped: no next store
    MwCtl* ctl;                // device; err is zero
};
struct tsq_mw_apply_out {
    int64_t addv, repv, addl, dropl;
    float ms;
};
// marks scanned -> k_mw_place_* -> lengths scanned to offsets -> k_mw_copy per cell family -> tsq_mv_index: the next store of m, a new
// writable handle (*next; NULL with null_when_unchanged when the records and marks change nothing).  
tsq_status tsq_mw_apply(tsq_mvcc* m, const tsq_mw_apply_in& in, tsq_mw_apply_out* out, tsq_mvcc** next);
// k_mw_copy: cell r of one family goes to cell didx[r] of dst (-1: nowhere); its bytes come from cell sidx[r] of the source (NULL: cell r;
// single: cell 0)
tsq_status tsq_mw_copy(tsq_ctx* ctx, tsq_handle_hdr* h, const uint8_t* src, const int64_t* soff, const int32_t* sidx, bool single, uint8_t* dst, const int64_t* doff,
                       const int32_t* didx, int64_t cnt);

// tsq_mvcc.hip.  A new handle with its events; errors go to ch.
tsq_status tsq_mv_new(tsq_ctx* ctx, tsq_handle_hdr* ch, std::unique_ptr<tsq_mvcc>* out);
// The store's arrays and counts are in m: the create checks, then the head flags, ordinals, segment starts and the key universe.
// internal: the arrays are the library's own (a write's next store) — a failed check is TSQ_ERR_HIP "internal: ...".
tsq_status tsq_mv_index(tsq_mvcc* m, tsq_handle_hdr* ch, bool internal);
void tsq_mv_store_view(const tsq_mvcc* m, tsq_mv_store* s);
tsq_status tsq_mv_copy_in(tsq_ctx* ctx, tsq_handle_hdr* h, DevBuf& b, const void* src, size_t bytes, bool dev, size_t at = 0, size_t room = 0);

#endif
