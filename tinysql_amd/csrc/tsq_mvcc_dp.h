// tsq_mvcc_dp.h — the per-key and per-cell code of the MVCC snapshot read (tsq_mvcc.hip): the checks of one stored version and one
// lock at create, the bound search of a range over the store's distinct keys, the lock check, and the walk of one key's versions —
// by one lane, and in the 64-entry steps a whole wave takes for a long chain.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/mvcc_dp_main.cpp): a read past a key,
// a chain or a level is found there, not on the GPU.
// Reference: store/mockstore/mocktikv — getValue (mvcc_leveldb.go:280-312), Scan / ReverseScan (:315-430), mvccLock.check
// (mvcc.go:197-207), mvccEntry.Get (mvcc.go:213-227).  Keys order as bytes.Compare; timestamps are unsigned 64-bit.
//
// The KEY UNIVERSE of a store is every distinct key that has a version or a lock, ascending: a lock on a key without versions is a
// key of its own (the reference's iterator stops at its lock entry and getValue checks it).  Key u is bytes
// [beg[u], beg[u] + len[u]) of `bytes` (the store's keys followed by the locks' keys), its versions are entries
// [seg[u], seg[u] + cnt[u]) in descending commitTS (a lock alone: cnt[u] = 0 and seg[u] is where its versions would go), lock[u] is
// its lock's index or -1.
// Every index below is bounded by the counts of the view alone (n, cnt), never by the data.
#ifndef TSQ_MVCC_DP_H
#define TSQ_MVCC_DP_H

#include "tsq_dupcheck_dp.h"  // tsq_dc_key_cmp, tsq_dc_bytes_equal: bytes.Compare / bytes.Equal over 8-byte pieces

// bits of the create checks (several may be set; mv_create_message of tsq_mvcc.hip picks the message in its own order)
#define TSQ_MV_E_OFFSETS 1u        // an offset pair that decreases or leaves its buffer
#define TSQ_MV_E_EMPTY_KEY 2u
#define TSQ_MV_E_KEY_ORDER 4u      // keys not ascending
#define TSQ_MV_E_VERSION_ORDER 8u  // versions of one key not descending in commitTS
#define TSQ_MV_E_EMPTY_PUT 16u     // a typePut with an empty value
#define TSQ_MV_E_TYPE 32u          // a value type or a lock op outside its enum
#define TSQ_MV_E_LOCK_ORDER 64u    // lock keys not ascending
#define TSQ_MV_E_LOCK_TWICE 128u   // two locks on one key

// offs[i] .. offs[i + 1] lies in [0, n_bytes] and does not decrease
TSQ_HD bool tsq_mv_pair_ok(const int64_t* offs, int64_t i, int64_t n_bytes) {
    const int64_t b = offs[i], t = offs[i + 1];
    return b >= 0 && b <= t && t <= n_bytes;
}

// entry i of the store against entry i - 1: its error bits; *head = it starts a new key.  Reads the keys of both entries only after
// their offset pairs were checked.
TSQ_HD uint32_t tsq_mv_entry_check(const uint8_t* keys, const int64_t* koff, int64_t key_bytes, const uint64_t* cts, const uint8_t* types,
                                   const int64_t* voff, int64_t value_bytes, int64_t i, bool* head) {
    *head = true;
    if (!tsq_mv_pair_ok(koff, i, key_bytes) || !tsq_mv_pair_ok(voff, i, value_bytes)) return TSQ_MV_E_OFFSETS;
    uint32_t e = 0;
    const int64_t b = koff[i], len = koff[i + 1] - b;
    if (len == 0) e |= TSQ_MV_E_EMPTY_KEY;
    const uint8_t t = types[i];
    if (t > TSQ_MVCC_ROLLBACK) e |= TSQ_MV_E_TYPE;
    if (t == TSQ_MVCC_PUT && voff[i + 1] == voff[i]) e |= TSQ_MV_E_EMPTY_PUT;
    if (i > 0) {
        if (!tsq_mv_pair_ok(koff, i - 1, key_bytes)) return e | TSQ_MV_E_OFFSETS;
        const int64_t pb = koff[i - 1];
        const int c = tsq_dc_key_cmp(keys + pb, b - pb, keys + b, len);
        if (c > 0) e |= TSQ_MV_E_KEY_ORDER;
        if (c == 0) {
            *head = false;
            if (!(cts[i] < cts[i - 1])) e |= TSQ_MV_E_VERSION_ORDER;
        }
    }
    return e;
}
// lock j against lock j - 1
TSQ_HD uint32_t tsq_mv_lock_entry_check(const uint8_t* lkeys, const int64_t* lkoff, int64_t lkey_bytes, const uint8_t* ops, const int64_t* lpoff,
                                        int64_t lprim_bytes, int64_t j) {
    if (!tsq_mv_pair_ok(lkoff, j, lkey_bytes) || !tsq_mv_pair_ok(lpoff, j, lprim_bytes)) return TSQ_MV_E_OFFSETS;
    uint32_t e = 0;
    const int64_t b = lkoff[j], len = lkoff[j + 1] - b;
    if (len == 0) e |= TSQ_MV_E_EMPTY_KEY;
    if (ops[j] > TSQ_MVCC_OP_ROLLBACK) e |= TSQ_MV_E_TYPE;
    if (j > 0) {
        if (!tsq_mv_pair_ok(lkoff, j - 1, lkey_bytes)) return e | TSQ_MV_E_OFFSETS;
        const int64_t pb = lkoff[j - 1];
        const int c = tsq_dc_key_cmp(lkeys + pb, b - pb, lkeys + b, len);
        if (c > 0) e |= TSQ_MV_E_LOCK_ORDER;
        if (c == 0) e |= TSQ_MV_E_LOCK_TWICE;
    }
    return e;
}

// first k in [0, K) whose key — the key of entry seg[k] — is >= the probe, K when there is none (create: a lock's place among the
// keys that have versions)
TSQ_HD int64_t tsq_mv_lower_heads(const uint8_t* keys, const int64_t* koff, const int32_t* seg, int64_t K, const uint8_t* probe, int64_t plen) {
    int64_t lo = 0, hi = K;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        const int64_t e = seg[mid], b = koff[e];
        if (tsq_dc_key_cmp(keys + b, koff[e + 1] - b, probe, plen) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct tsq_mv_keys {
    const uint8_t* bytes;
    const int64_t* beg;  // [n]
    const int32_t* len;  // [n]
    int64_t n;
};
// first u in [0, n) with key u >= the probe, n when there is none
TSQ_HD int64_t tsq_mv_lower(const tsq_mv_keys& k, const uint8_t* probe, int64_t plen) {
    int64_t lo = 0, hi = k.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tsq_dc_key_cmp(k.bytes + k.beg[mid], k.len[mid], probe, plen) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// the key ordinals [*lo, *lo + *cnt) of one range.  [start, end): an empty start is the first key, an empty end the last one,
// start >= end selects nothing.  TSQ_MVCC_POINT: Get(start) — the key equal to start alone (getRowFromPoint, executor.go:271-320);
// keys that merely extend it do not count, an empty start finds nothing.
TSQ_HD void tsq_mv_bounds(const tsq_mv_keys& k, const uint8_t* start, int64_t slen, const uint8_t* end, int64_t elen, uint32_t flags, int64_t* lo,
                          int64_t* cnt) {
    const int64_t a = slen > 0 ? tsq_mv_lower(k, start, slen) : 0;
    *lo = a;
    if (flags & TSQ_MVCC_POINT) {
        *cnt = (slen > 0 && a < k.n && tsq_dc_bytes_equal(k.bytes + k.beg[a], k.len[a], start, slen)) ? 1 : 0;
        return;
    }
    const int64_t b = elen > 0 ? tsq_mv_lower(k, end, elen) : k.n;
    *cnt = b > a ? b - a : 0;
}

// The position space of a scan: the ranges' intervals one after the other, base[r] = the positions before range r (R + 1 entries,
// base[R] = all).  The range of position p (0 <= p < base[R]): the last r with base[r] <= p — empty ranges are stepped over.
TSQ_HD int64_t tsq_mv_range_of(const int64_t* base, int64_t R, int64_t p) {
    int64_t lo = 0, hi = R;  // first r in [0, R] with base[r] > p, minus one
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (base[mid] <= p) lo = mid + 1;
        else hi = mid;
    }
    return lo - 1;
}
// position j of a range's interval: from the bottom, or for a descending scan from the top
TSQ_HD int64_t tsq_mv_key_at(int64_t lo, int64_t cnt, int64_t j, int desc) { return desc ? lo + cnt - 1 - j : lo + j; }
// first i in [0, n) with v[i] >= x (ascending int64), n when there is none
TSQ_HD int64_t tsq_mv_lower_i64(const int64_t* v, int64_t n, int64_t x) {
    int64_t lo = 0, hi = n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (v[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

struct tsq_mv_store {
    tsq_mv_keys k;
    const int32_t* seg;   // [k.n] first entry of the key's versions
    const int32_t* cnt;   // [k.n] versions of the key (0: a lock alone)
    const int32_t* lock;  // [k.n] the key's lock or -1
    const uint64_t* cts;  // per entry
    const uint8_t* types;
    const uint64_t* l_start;  // per lock
    const uint8_t* l_op;
    const uint8_t* l_prim;
    const int64_t* l_poff;
};

// mvccLock.check (mvcc.go:197-207) on key u at *ts: 0 = the read goes on at *ts, 1 = ErrLocked.  A lock is ignored when it is younger
// than the read or a mere Op_Lock; the read of the latest version (ts = 2^64 - 1) of the lock's own primary goes on at startTS - 1
// (unsigned: a startTS of 0 wraps to 2^64 - 1, as Go's uint64 does).
TSQ_HD int tsq_mv_key_lock(const tsq_mv_store& s, int64_t u, uint64_t* ts) {
    const int32_t j = s.lock[u];
    if (j < 0) return 0;
    const uint64_t ls = s.l_start[j];
    if (ls > *ts || s.l_op[j] == TSQ_MVCC_OP_LOCK) return 0;
    if (*ts == UINT64_MAX) {
        const int64_t pb = s.l_poff[j];
        if (tsq_dc_bytes_equal(s.l_prim + pb, s.l_poff[j + 1] - pb, s.k.bytes + s.k.beg[u], s.k.len[u])) {
            *ts = ls - 1;
            return 0;
        }
    }
    return 1;
}

// first i in [s, e) with cts[i] <= ts — versions are in descending commitTS, so those a read at ts cannot see are skipped by a search
TSQ_HD int64_t tsq_mv_first_le(const uint64_t* cts, int64_t s, int64_t e, uint64_t ts, int64_t* walked) {
    while (s < e) {
        const int64_t mid = s + ((e - s) >> 1);
        (*walked)++;
        if (cts[mid] > ts) s = mid + 1;
        else e = mid;
    }
    return s;
}
// what entry i says once it decides: the pair of a put, nothing for a delete
TSQ_HD int64_t tsq_mv_verdict(const uint8_t* types, int64_t i) { return types[i] == TSQ_MVCC_PUT ? i : -1; }
// getValue's loop on entries [s, e) by one lane: the first version with commitTS <= ts that is not a rollback decides; -1: no pair
TSQ_HD int64_t tsq_mv_walk(const uint64_t* cts, const uint8_t* types, int64_t s, int64_t e, uint64_t ts, int64_t* walked) {
    int64_t i = tsq_mv_first_le(cts, s, e, ts, walked);
    while (i < e && types[i] == TSQ_MVCC_ROLLBACK) {
        i++;
        (*walked)++;
    }
    return i < e ? tsq_mv_verdict(types, i) : -1;
}
// the wave form: after tsq_mv_first_le the wave looks at 64 entries per step, lane l at entry i0 + l; the first lane for which this
// holds names the deciding entry
TSQ_HD bool tsq_mv_decides(const uint8_t* types, int64_t i, int64_t e) { return i < e && types[i] != TSQ_MVCC_ROLLBACK; }

#endif
