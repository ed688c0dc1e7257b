// tsq_unionstore_dp.h — the per-position code of a transaction's merged read (tsq_unionstore.hip): where a snapshot position and a
// buffer position of one range go among the range's merged candidates, which of them yields a pair, the verdict of one point key,
// and the lock decision of a call.  The bounds, the per-key resolve and the lock check are tsq_mvcc_dp.h's, the buffer's bounds
// tsq_memread_dp.h's, the key compare tsq_dupcheck_dp.h's: nothing of them is restated here.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/unionstore_dp_main.cpp).
// Reference: kv/union_iter.go updateCur (:64-137) and Next (:140-152), kv/buffer_store.go Get (:61-73), Iter / IterReverse (:76-99).
//
// The CANDIDATES of range r are its snapshot positions (the keys of the store's key universe inside the range, sbase[r] ..
// sbase[r + 1]) and its buffer positions (the finished buffer's entries inside the range, bbase[r] .. bbase[r + 1]), both in scan
// direction.  Range r owns the candidate slots [sbase[r] + bbase[r], sbase[r + 1] + bbase[r + 1]); inside them the candidates stand
// in merged order, a snapshot key BEFORE the buffer entry of the same key — so the pairs in front of a snapshot key's slot are the
// merged pairs before that key, whatever the buffer says about the key itself.  A slot is the position's own index in its side plus
// the number of the other side's keys in front of it: one bound search per position, no position waits for another.
// Every index below is bounded by the counts of the two views and of the call, never by the data.
#ifndef TSQ_UNIONSTORE_DP_H
#define TSQ_UNIONSTORE_DP_H

#include "tsq_memread_dp.h"
#include "tsq_mvcc_dp.h"

#define TSQ_UN_E_OFFSETS 1u   // an offset pair of the call that decreases or leaves its buffer
#define TSQ_UN_E_INTERNAL 2u  // a slot outside its range's candidates: nothing is written there

// Snapshot position j (in scan direction) of a range whose buffer entries are [blo, blo + bcnt): its slot among the range's
// candidates; *shadow = the buffer holds the key as PUT or DEL (a lock-only entry shadows nothing).
TSQ_HD int64_t tsq_un_snapshot_slot(const tsq_mr_buffer& b, int64_t blo, int64_t bcnt, const uint8_t* key, int64_t klen, int64_t j, int desc, bool* shadow) {
    *shadow = false;
    if (bcnt <= 0) return j;
    int64_t e = tsq_dc_key_lower(b.okeys, b.okoff, b.m, key, klen);
    e = e < blo ? blo : (e > blo + bcnt ? blo + bcnt : e);  // (the key lies inside the range, so its bound does: checked, not assumed)
    const bool eq = e < blo + bcnt && e < b.m && tsq_dc_bytes_equal(b.okeys + b.okoff[e], b.okoff[e + 1] - b.okoff[e], key, klen);
    *shadow = eq && b.oops[e] != TSQ_MVCC_OP_LOCK;
    return desc ? j + (blo + bcnt - e - (eq ? 1 : 0)) : j + (e - blo);
}

// Buffer position i (in scan direction) of a range whose snapshot keys are the ordinals [slo, slo + scnt) and whose buffer entries
// are [blo, blo + bcnt): its entry, its slot, and *snap_j = the snapshot position (in scan direction, inside the range) of the same
// key or -1.
TSQ_HD int64_t tsq_un_buffer_slot(const tsq_mr_buffer& b, const tsq_mv_keys& k, int64_t slo, int64_t scnt, int64_t blo, int64_t bcnt, int64_t i, int desc,
                                  int64_t* entry, int64_t* snap_j) {
    const int64_t e = desc ? blo + bcnt - 1 - i : blo + i;
    *entry = e;
    *snap_j = -1;
    if (scnt <= 0) return i;
    const uint8_t* key = b.okeys + b.okoff[e];
    const int64_t klen = b.okoff[e + 1] - b.okoff[e];
    int64_t a = tsq_mv_lower(k, key, klen);
    a = a < slo ? slo : (a > slo + scnt ? slo + scnt : a);
    const bool eq = a < slo + scnt && a < k.n && tsq_dc_bytes_equal(k.bytes + k.beg[a], k.len[a], key, klen);
    if (eq) *snap_j = desc ? slo + scnt - 1 - a : a - slo;
    return desc ? i + (slo + scnt - a) : i + (a - slo) + (eq ? 1 : 0);
}

// what a candidate yields: a snapshot position its visible pair unless the buffer shadows the key; a buffer position its PUT
TSQ_HD bool tsq_un_keep_snapshot(int64_t chosen, bool shadow) { return chosen >= 0 && !shadow; }
TSQ_HD bool tsq_un_keep_buffer(uint8_t op) { return op == TSQ_MVCC_OP_PUT; }

// The source of a pair in one int32: a store entry as it is, a buffer entry e as ~e
TSQ_HD int32_t tsq_un_src_buffer(int64_t e) { return (int32_t)~e; }
TSQ_HD bool tsq_un_src_is_buffer(int32_t s) { return s < 0; }
TSQ_HD int64_t tsq_un_src_entry(int32_t s) { return s < 0 ? (int64_t)~s : (int64_t)s; }

// The lock decision of a range read.  L is the FIRST locked snapshot position of the call, in range r.  The snapshot iterator steps
// onto L when it leaves the visible snapshot pair in front of L in the same range (`prev`) or, without one, when the range is
// opened.  It leaves prev when the buffer holds prev's key (updateCur steps both sides as soon as they meet, union_iter.go:98-115:
// that needs the merged pairs before the key to be taken and one more Next — before_prev < limit) or when prev was yielded and the
// consumer asked for more (before_prev + 1 < limit).  A range is opened while fewer than `limit` pairs are taken.
// -> the lock is met; *n_pairs = the pairs taken before the error.
TSQ_HD bool tsq_un_lock_met(bool has_prev, int64_t before_prev, bool prev_shadowed, int64_t before_range, int64_t limit, int64_t* n_pairs) {
    const int64_t c = has_prev ? before_prev + (prev_shadowed ? 0 : 1) : before_range;
    *n_pairs = c;
    return c < limit;
}

// the verdicts of one point key
#define TSQ_UN_PT_NONE 0      // ErrNotExist: neither side yields the key
#define TSQ_UN_PT_BUFFER 1    // the buffer's PUT (*src = its entry)
#define TSQ_UN_PT_DELETED 2   // the buffer's DEL: ErrNotExist WITHOUT reading the snapshot — a lock on the key is not met
#define TSQ_UN_PT_SNAPSHOT 3  // the snapshot's pair (*src = the store entry)
#define TSQ_UN_PT_LOCKED 4    // the snapshot's Get met a lock (*src = the key's ordinal)
// BufferStore.Get of key i, passed as in a push (koff NULL: keys of fixed_len bytes)
TSQ_HD int tsq_un_point(const tsq_mr_buffer& b, const tsq_mv_store& s, const uint8_t* keys, const int64_t* koff, int64_t fixed_len, int64_t key_bytes, int64_t i,
                        uint64_t ts, int64_t* src, int64_t* walked, uint32_t* err) {
    *src = -1;
    uint32_t e0 = 0;
    int64_t held = 0;
    const int64_t e = tsq_mr_point(b, keys, koff, fixed_len, key_bytes, i, &held, &e0);
    if (e0) {
        *err |= TSQ_UN_E_OFFSETS;
        return TSQ_UN_PT_NONE;
    }
    if (held) {
        const uint8_t op = b.oops[e];
        if (op == TSQ_MVCC_OP_PUT) {
            *src = e;
            return TSQ_UN_PT_BUFFER;
        }
        if (op == TSQ_MVCC_OP_DEL) return TSQ_UN_PT_DELETED;
    }
    const int64_t kb = koff ? koff[i] : i * fixed_len, kl = koff ? koff[i + 1] - koff[i] : fixed_len;
    int64_t u = 0, cnt = 0;
    tsq_mv_bounds(s.k, keys + kb, kl, keys + kb, 0, TSQ_MVCC_POINT, &u, &cnt);
    if (cnt == 0) return TSQ_UN_PT_NONE;
    if (tsq_mv_key_lock(s, u, &ts)) {
        *src = u;
        return TSQ_UN_PT_LOCKED;
    }
    const int64_t first = s.seg[u];
    const int64_t ch = tsq_mv_walk(s.cts, s.types, first, first + s.cnt[u], ts, walked);
    if (ch < 0) return TSQ_UN_PT_NONE;
    *src = ch;
    return TSQ_UN_PT_SNAPSHOT;
}

#endif
