// tsq_mvcc_maint_dp.h — the per-lock, per-key and per-entry code of the range calls of an MVCC store (tsq_mvcc_maint.hip): a key range
// as bounds in the key universe, among the version entries and among the locks; ScanLock's test of one lock; ResolveLock's decision
// on one lock and the place of the version it adds; GC's two indices per key — by one lane, and the keeper's walk in the 64-entry steps
// a whole wave takes — and its drop test per entry.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/mvcc_maint_dp_main.cpp).
// Reference: store/mockstore/mocktikv/mvcc_leveldb.go — newScanIterator (:149-171), ScanLock (:906-939), ResolveLock (:942-978),
// BatchResolveLock (:981-1019), GC (:1022-1085), DeleteRange (:1088-1090, :1231-1246), commitLock (:590-613), rollbackLock (:686-700).
// Timestamps compare unsigned.
// Every index below is bounded by the counts of the store view (n, n_locks, k.n, cnt, K) and of the transaction list, never by the data.
#ifndef TSQ_MVCC_MAINT_DP_H
#define TSQ_MVCC_MAINT_DP_H

#include "tsq_mvcc_write_dp.h"

// a key range in the three index spaces of a store: keys [u0, u1) of the universe, version entries [e0, e1), locks [l0, l1)
struct tsq_mm_bounds {
    int64_t u0, u1, e0, e1, l0, l1;
};
// [start, end) with newScanIterator's meaning (tsq_mv_bounds: an empty start is the first key, an empty end the last one, start >= end
// selects nothing).  A key's entries begin at seg[u] — for a key that is a lock alone, where its versions would go — so the entries of
// keys [u0, u1) are [seg[u0], seg[u1]) with seg[k.n] = n; the locks by the same two searches over the locks' keys.
TSQ_HD void tsq_mm_range(const tsq_mw_store& st, const uint8_t* start, int64_t slen, const uint8_t* end, int64_t elen, tsq_mm_bounds* b) {
    int64_t lo = 0, cnt = 0;
    tsq_mv_bounds(st.s.k, start, slen, end, elen, 0u, &lo, &cnt);
    b->u0 = lo;
    b->u1 = lo + cnt;
    b->e0 = b->u0 < st.s.k.n ? (int64_t)st.s.seg[b->u0] : st.n;
    b->e1 = b->u1 < st.s.k.n ? (int64_t)st.s.seg[b->u1] : st.n;
    b->l0 = slen > 0 ? tsq_mw_lower_cells(st.lkeys, st.lkoff, st.n_locks, start, slen) : 0;
    b->l1 = elen > 0 ? tsq_mw_lower_cells(st.lkeys, st.lkoff, st.n_locks, end, elen) : st.n_locks;
    if (cnt == 0) b->e1 = b->e0, b->l1 = b->l0;  // (start >= end)
    if (b->e1 < b->e0) b->e1 = b->e0;
    if (b->l1 < b->l0) b->l1 = b->l0;
}

// ScanLock (:923) and GC's refusal (:1041): lock j is at or under the timestamp
TSQ_HD bool tsq_mm_lock_le(const uint64_t* l_start, int64_t j, uint64_t ts) { return l_start[j] <= ts; }

// the transaction with this start_ts in the list sorted by start_ts (unsigned, no duplicates), or -1
TSQ_HD int64_t tsq_mm_find_txn(const uint64_t* txn_start, int64_t T, uint64_t ts) {
    int64_t lo = 0, hi = T;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (txn_start[mid] < ts) lo = mid + 1;
        else hi = mid;
    }
    return lo < T && txn_start[lo] == ts ? lo : -1;
}
// ResolveLock / BatchResolveLock on lock j (:959-964, :999-1004): its transaction is in the list — the lock goes; commit_ts > 0:
// commitLock (:590-613), op != Op_Lock adds (PUT | DELETE, the lock's startTS, commit_ts, the lock's value); commit_ts == 0:
// rollbackLock (:686-700) adds (ROLLBACK, startTS, commitTS = startTS, empty).  The new version's place in the key's chain is
// tsq_mw_insert_at's — a binary search over [s, e); an equal commitTS is replaced.  o->vcts: the new version's commitTS.
// Returns whether the lock was resolved.
TSQ_HD bool tsq_mm_resolve(const tsq_mw_store& st, int64_t j, const uint64_t* txn_start, const uint64_t* txn_commit, int64_t T, tsq_mw_plan* o) {
    tsq_mw_plan_none(o);
    const uint64_t ls = st.s.l_start[j];
    const int64_t t = tsq_mm_find_txn(txn_start, T, ls);
    if (t < 0) return false;
    o->flags = TSQ_MW_DROP_LOCK;
    o->lpos = (int32_t)j;
    const uint64_t c = txn_commit[t];
    const uint8_t op = st.s.l_op[j];
    if (c > 0 && op == TSQ_MVCC_OP_LOCK) return true;  // (:595) no version
    tsq_mw_place p;
    const int64_t kb = st.lkoff[j];
    tsq_mw_locate(st, st.lkeys + kb, st.lkoff[j + 1] - kb, &p);
    if (c > 0) tsq_mw_add_version(st, p, c, op == TSQ_MVCC_OP_PUT ? TSQ_MVCC_PUT : TSQ_MVCC_DELETE, (int32_t)j, o);
    else tsq_mw_add_version(st, p, ls, TSQ_MVCC_ROLLBACK, -1, o);
    return true;
}

// GC on the chain [s, e) of one key (:1052-1080).  lo: the first entry with commitTS <= safe_point (the entries before it stay, :1067).
TSQ_HD int64_t tsq_mm_gc_lo(const uint64_t* cts, int64_t s, int64_t e, uint64_t safe_point) {
    int64_t walked = 0;
    return tsq_mv_first_le(cts, s, e, safe_point, &walked);
}
// the first PUT-or-DELETE of [lo, e) by one lane, or -1 (the wave form: tsq_mv_decides per lane, the first lane for which it holds)
TSQ_HD int64_t tsq_mm_gc_first(const uint8_t* types, int64_t lo, int64_t e) {
    for (int64_t i = lo; i < e; i++)
        if (types[i] != TSQ_MVCC_ROLLBACK) return i;
    return -1;
}
// the keeper: that entry stays iff it is a PUT (:1073); -1: none of [lo, e) stays
TSQ_HD int64_t tsq_mm_gc_keeper(const uint8_t* types, int64_t first) { return first >= 0 && types[first] == TSQ_MVCC_PUT ? first : -1; }
// entry p of a key with (lo, keeper) goes
TSQ_HD bool tsq_mm_gc_drops(int64_t p, int64_t lo, int64_t keeper) { return p >= lo && p != keeper; }

#endif
