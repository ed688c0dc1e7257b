// tsq_mvcc_write_dp.h — the per-key code of the MVCC writes (tsq_mvcc_write.hip): the checks of one request key, its place in the
// store, the verdict of Prewrite / Commit / Rollback on it, and what the apply does for it — by one lane; the walk of a long chain
// for the version of a transaction also in the 64-entry steps a whole wave takes.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/mvcc_write_dp_main.cpp).
// Reference: store/mockstore/mocktikv/mvcc_leveldb.go — prewriteMutation (:493-537), commitKey / commitLock (:560-613),
// rollbackKey / rollbackLock (:634-700), getTxnCommitInfo (:702-717).  Timestamps compare unsigned.
// Every index below is bounded by the counts of the store view and of the request, never by the data.
#ifndef TSQ_MVCC_WRITE_DP_H
#define TSQ_MVCC_WRITE_DP_H

#include "tsq_mvcc_dp.h"

#define TSQ_MW_PREWRITE 0
#define TSQ_MW_COMMIT 1
#define TSQ_MW_ROLLBACK 2

// bits of the request checks (mw_request_message of tsq_mvcc_write.hip picks the message in its own order)
#define TSQ_MW_E_OFFSETS 1u    // an offset pair that decreases or leaves its buffer
#define TSQ_MW_E_EMPTY_KEY 2u
#define TSQ_MW_E_ORDER 4u      // keys not strictly ascending
#define TSQ_MW_E_OP 8u         // a prewrite op other than Put / Del / Lock
#define TSQ_MW_E_EMPTY_PUT 16u

// what the apply does for one key
#define TSQ_MW_ADD_VERSION 1u   // a new version at entry index vpos of the current store (before the entry that is there)
#define TSQ_MW_REP_VERSION 2u   // ... and the entry at vpos, which has the same (key, commitTS), goes
#define TSQ_MW_ADD_LOCK 4u      // a new lock at lock index lpos
#define TSQ_MW_DROP_LOCK 8u     // the lock at lpos goes

// the current store as a write sees it: the read view plus the entries' startTS and the locks' keys
struct tsq_mw_store {
    tsq_mv_store s;
    const uint64_t* sts;   // [n]
    int64_t n;
    const uint8_t* lkeys;  // the locks' keys
    const int64_t* lkoff;  // [n_locks + 1]
    int64_t n_locks;
};
struct tsq_mw_req {
    const uint8_t* keys;
    const int64_t* koff;  // [q + 1]
    int64_t key_bytes;
    int64_t q;
    const uint8_t* ops;   // prewrite: [q]
    const int64_t* voff;  // prewrite: [q + 1]
    int64_t value_bytes;
    int32_t kind;         // TSQ_MW_*
    uint64_t start_ts;
    uint64_t commit_ts;
};
struct tsq_mw_place {  // key i in the store
    int64_t u;         // its lower bound in the key universe
    bool eq;           // it is that key
    int32_t lock;      // its lock or -1
    int64_t s, e;      // its versions, entries [s, e); a key without versions: s == e == where its first version would go
};
struct tsq_mw_plan {
    uint8_t verdict;   // TSQ_MVCC_V_*
    uint8_t flags;     // TSQ_MW_ADD_VERSION ...
    uint8_t vtype;     // the new version's type
    int32_t vsrc;      // the lock whose value becomes the new version's value, or -1: empty
    int32_t vpos, lpos;
    uint64_t vcts;     // the new version's commitTS
    uint64_t info0, info1;
};

// key i of the request against key i - 1: its error bits.  Reads the keys of both only after their offset pairs were checked.
TSQ_HD uint32_t tsq_mw_req_check(const tsq_mw_req& r, int64_t i) {
    if (!tsq_mv_pair_ok(r.koff, i, r.key_bytes)) return TSQ_MW_E_OFFSETS;
    if (r.kind == TSQ_MW_PREWRITE && !tsq_mv_pair_ok(r.voff, i, r.value_bytes)) return TSQ_MW_E_OFFSETS;
    uint32_t e = 0;
    const int64_t b = r.koff[i], len = r.koff[i + 1] - b;
    if (len == 0) e |= TSQ_MW_E_EMPTY_KEY;
    if (r.kind == TSQ_MW_PREWRITE) {
        const uint8_t op = r.ops[i];
        if (op > TSQ_MVCC_OP_LOCK) e |= TSQ_MW_E_OP;
        if (op == TSQ_MVCC_OP_PUT && r.voff[i + 1] == r.voff[i]) e |= TSQ_MW_E_EMPTY_PUT;
    }
    if (i > 0) {
        if (!tsq_mv_pair_ok(r.koff, i - 1, r.key_bytes)) return e | TSQ_MW_E_OFFSETS;
        const int64_t pb = r.koff[i - 1];
        if (tsq_dc_key_cmp(r.keys + pb, b - pb, r.keys + b, len) >= 0) e |= TSQ_MW_E_ORDER;
    }
    return e;
}

// first cell in [0, n) that is >= the probe, n when there is none (a new lock's place among the locks' keys)
TSQ_HD int64_t tsq_mw_lower_cells(const uint8_t* keys, const int64_t* koff, int64_t n, const uint8_t* probe, int64_t plen) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t b = koff[mid];
        if (tsq_dc_key_cmp(keys + b, koff[mid + 1] - b, probe, plen) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

TSQ_HD void tsq_mw_locate(const tsq_mw_store& st, const uint8_t* key, int64_t len, tsq_mw_place* p) {
    const int64_t u = tsq_mv_lower(st.s.k, key, len);
    p->u = u;
    p->eq = u < st.s.k.n && tsq_dc_bytes_equal(st.s.k.bytes + st.s.k.beg[u], st.s.k.len[u], key, len);
    p->lock = p->eq ? st.s.lock[u] : -1;
    // (the entries of keys >= the probe start where key u's do — for a key that is a lock alone, where its versions would go)
    const int64_t s = u < st.s.k.n ? (int64_t)st.s.seg[u] : st.n;
    p->s = s;
    p->e = s + (p->eq ? (int64_t)st.s.cnt[u] : 0);
}

// does the verdict of key i need the version of the transaction (getTxnCommitInfo's walk)?  Commit and Rollback without the
// transaction's own lock on the key.
TSQ_HD bool tsq_mw_needs_walk(const tsq_mw_store& st, const tsq_mw_req& r, const tsq_mw_place& p) {
    if (r.kind == TSQ_MW_PREWRITE) return false;
    return !(p.lock >= 0 && st.s.l_start[p.lock] == r.start_ts);
}
// the first entry of [s, e) with start_ts == ts, by one lane; -1: none
TSQ_HD int64_t tsq_mw_find_start(const uint64_t* sts, int64_t s, int64_t e, uint64_t ts) {
    for (int64_t i = s; i < e; i++)
        if (sts[i] == ts) return i;
    return -1;
}
// the wave form: lane l looks at entry i0 + l; the first lane for which this holds names the entry
TSQ_HD bool tsq_mw_is_start(const uint64_t* sts, int64_t i, int64_t e, uint64_t ts) { return i < e && sts[i] == ts; }

// where a version with commitTS c goes in the chain [s, e) (descending commitTS): the first i with cts[i] <= c; *rep: that entry
// has commitTS c itself and is replaced — (key, commitTS) is one LevelDB key
TSQ_HD int64_t tsq_mw_insert_at(const uint64_t* cts, int64_t s, int64_t e, uint64_t c, bool* rep) {
    int64_t lo = s, hi = e;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const bool newer = cts[mid] > c;
        lo = newer ? mid + 1 : lo;
        hi = newer ? hi : mid;
    }
    *rep = lo < e && cts[lo] == c;
    return lo;
}

TSQ_HD void tsq_mw_add_version(const tsq_mw_store& st, const tsq_mw_place& p, uint64_t c, uint8_t type, int32_t vsrc, tsq_mw_plan* o) {
    bool rep = false;
    o->vpos = (int32_t)tsq_mw_insert_at(st.s.cts, p.s, p.e, c, &rep);
    o->flags |= TSQ_MW_ADD_VERSION | (rep ? TSQ_MW_REP_VERSION : 0u);
    o->vtype = type;
    o->vsrc = vsrc;
    o->vcts = c;
}

TSQ_HD void tsq_mw_plan_none(tsq_mw_plan* o) {
    o->verdict = TSQ_MVCC_V_OK;
    o->flags = 0;
    o->vtype = 0;
    o->vsrc = -1;
    o->vpos = o->lpos = 0;
    o->vcts = 0;
    o->info0 = o->info1 = 0;
}
// the verdict of key i and its plan.  found: for a key that tsq_mw_needs_walk, the first entry of its chain with
// start_ts == r.start_ts or -1 (tsq_mw_find_start, or the wave's walk); otherwise not read.
TSQ_HD void tsq_mw_decide(const tsq_mw_store& st, const tsq_mw_req& r, int64_t i, const tsq_mw_place& p, int64_t found, tsq_mw_plan* o) {
    tsq_mw_plan_none(o);
    const int32_t j = p.lock;
    const bool own = j >= 0 && st.s.l_start[j] == r.start_ts;
    if (r.kind == TSQ_MW_PREWRITE) {
        if (j >= 0 && !own) {  // (:509-512) lockErr
            o->verdict = TSQ_MVCC_V_LOCKED;
            o->info0 = (uint64_t)j;
            return;
        }
        if (own) {  // (:509-518) the own lock is written again; checkConflictValue is not run
            o->flags = TSQ_MW_ADD_LOCK | TSQ_MW_DROP_LOCK;
            o->lpos = j;
            return;
        }
        // (:513-518, :472-491) the newest entry of the chain, whatever its type; a key without versions has commitTS 0
        const uint64_t c = p.e > p.s ? st.s.cts[p.s] : 0, s0 = p.e > p.s ? st.sts[p.s] : 0;
        if (c >= r.start_ts) {
            o->verdict = TSQ_MVCC_V_CONFLICT;
            o->info0 = s0;
            o->info1 = c;
            return;
        }
        const int64_t kb = r.koff[i];
        o->flags = TSQ_MW_ADD_LOCK;
        o->lpos = (int32_t)tsq_mw_lower_cells(st.lkeys, st.lkoff, st.n_locks, r.keys + kb, r.koff[i + 1] - kb);
        return;
    }
    if (r.kind == TSQ_MW_COMMIT) {
        if (own) {  // commitLock (:590-613)
            o->flags = TSQ_MW_DROP_LOCK;
            o->lpos = j;
            const uint8_t op = st.s.l_op[j];
            if (op != TSQ_MVCC_OP_LOCK) tsq_mw_add_version(st, p, r.commit_ts, op == TSQ_MVCC_OP_PUT ? TSQ_MVCC_PUT : TSQ_MVCC_DELETE, j, o);
            return;
        }
        // (:570-582) no lock of the transaction: committed already, or never prewritten / rolled back
        o->verdict = found >= 0 && st.s.types[found] != TSQ_MVCC_ROLLBACK ? TSQ_MVCC_V_NOOP : TSQ_MVCC_V_TXN_NOT_FOUND;
        return;
    }
    if (own) {  // (:648-653) rollbackLock (:686-700)
        o->flags = TSQ_MW_DROP_LOCK;
        o->lpos = j;
        tsq_mw_add_version(st, p, r.start_ts, TSQ_MVCC_ROLLBACK, -1, o);
        return;
    }
    if (found >= 0) {  // (:657-668)
        if (st.s.types[found] != TSQ_MVCC_ROLLBACK) {
            o->verdict = TSQ_MVCC_V_ALREADY_COMMITTED;
            o->info0 = st.s.cts[found];
        } else {
            o->verdict = TSQ_MVCC_V_NOOP;
        }
        return;
    }
    tsq_mw_add_version(st, p, r.start_ts, TSQ_MVCC_ROLLBACK, -1, o);  // (:671-683) a foreign lock stays
}

#endif
