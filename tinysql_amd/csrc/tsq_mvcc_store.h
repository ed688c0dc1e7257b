// tsq_mvcc_store.h — the handle of an MVCC store, shared by its two units: tsq_mvcc.hip (create, the snapshot reads) and
// tsq_mvcc_write.hip (the writable create, Prewrite / Commit / Rollback into the next store, the export).
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
};

// tsq_mvcc.hip.  A new handle with its events; errors go to ch.
tsq_status tsq_mv_new(tsq_ctx* ctx, tsq_handle_hdr* ch, std::unique_ptr<tsq_mvcc>* out);
// The store's arrays and counts are in m: the create checks, then the head flags, ordinals, segment starts and the key universe.
// internal: the arrays are the library's own (a write's next store) — a failed check is TSQ_ERR_HIP "internal: ...".
tsq_status tsq_mv_index(tsq_mvcc* m, tsq_handle_hdr* ch, bool internal);
void tsq_mv_store_view(const tsq_mvcc* m, tsq_mv_store* s);
tsq_status tsq_mv_copy_in(tsq_ctx* ctx, tsq_handle_hdr* h, DevBuf& b, const void* src, size_t bytes, bool dev, size_t at = 0, size_t room = 0);

#endif
