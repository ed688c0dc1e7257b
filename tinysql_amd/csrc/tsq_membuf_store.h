// tsq_membuf_store.h — the handle of a transaction buffer, shared by its units: tsq_membuf.hip (push, finish, request, Get) and
// tsq_memread.hip (the range scan, the point reads and the dirty handles of the finished buffer).
#ifndef TSQ_MEMBUF_STORE_H
#define TSQ_MEMBUF_STORE_H

#include "tsq_stage.h"

#define TSQ_MAGIC_MEMBUF 0x74737142u /* 'tsqB' */

struct tsq_membuf {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    tsq_membuf_cfg cfg;
    // the entries by sequence number
    int64_t n = 0, key_used = 0, val_used = 0;
    DevBuf keys, vals, kbeg, klen, vbeg, vlen, kind;
    // the request of the last finish
    bool finished = false;
    int64_t finishes = 0;  // counts the finishes: a reader of the arrays below (tsq_unionstore.hip) tells by it that they are still the ones it scanned
    int64_t m = 0, okey_bytes = 0, oval_bytes = 0;
    DevBuf okeys, okoff, oops, ovals, ovoff;
    DevBuf ctl;
    DevEvent ev[2];
    // the last tsq_membuf_scan / tsq_membuf_scan_points (tsq_memread.hip): per range its first entry and (scanned) its first position;
    // per position its entry and (scanned) the pair ordinal and the two byte offsets.  A push or a finish forgets it.
    DevBuf mr_rng, mr_roff, mr_rlo, mr_rbase, mr_entry, mr_ord, mr_koff, mr_voff, mr_rc, mr_tmp, mr_ctl;
    bool mr_have = false;
    int32_t mr_desc = 0;
    int64_t mr_positions = 0, mr_pairs = 0, mr_key_bytes = 0, mr_value_bytes = 0;
    // the last tsq_membuf_dirty: per entry of the table's record range its handle and (scanned) its place in either list
    DevBuf dt_handle, dt_added, dt_deleted;
    bool dt_have = false;
    int64_t dt_positions = 0, dt_n_added = 0, dt_n_deleted = 0;
    void forget_reads() { mr_have = dt_have = false; }
};

#endif
