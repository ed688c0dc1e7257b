// tsq_unionscan_dp.h — the scalar core of UnionScan (tsq_unionscan.hip): the dirty-handle set (build and probe), the row comparator
// of UnionScanExec.compare, the merge-path diagonal search, the cut of a tile out of both runs and the sequential merge one lane runs on its stretch of the tile.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/unionscan_dp_main.cpp): an index that
// leaves its array is found there, not on the GPU.
// Reference: executor/union_scan.go — getSnapshotRow :198-225 (the two set look-ups), getOneRow :160-196, shouldPickFirstRow
// :237-254, compare :256-280; CompareDatum's orders as tsq_sort_image.h encodes them.
#ifndef TSQ_UNIONSCAN_DP_H
#define TSQ_UNIONSCAN_DP_H

#include "tsq_device.h"
#include "tsq_sort_image.h"

// ---------------------------------------------------------------- the handle set
// Open addressing, linear probing, at most half full.  Every int64 is a legal handle, so a free slot is not marked by a key value:
// bit s of `occ` says that slot s holds a key.
struct tsq_us_set {
    const uint64_t* keys;  // [slots]
    const uint32_t* occ;   // [slots / 32]
    uint64_t slots;        // a power of two >= 64; 0: the empty set, nothing is probed
};
TSQ_HD uint64_t tsq_us_set_slots(uint64_t n_handles) {
    if (n_handles == 0) return 0;
    uint64_t s = 64;
    while (s < 2 * n_handles) s <<= 1;
    return s;
}
TSQ_HD uint64_t tsq_us_slot(uint64_t handle, uint64_t slots) { return tsq_mix64(handle) & (slots - 1); }
// host-side build (keys / occ zeroed, writable); a handle already there is not stored twice
TSQ_HD void tsq_us_set_insert(uint64_t* keys, uint32_t* occ, uint64_t slots, uint64_t handle) {
    uint64_t s = tsq_us_slot(handle, slots);
    for (uint64_t step = 0; step < slots; step++) {
        if (!((occ[s >> 5] >> (s & 31)) & 1u)) {
            keys[s] = handle;
            occ[s >> 5] |= 1u << (s & 31);
            return;
        }
        if (keys[s] == handle) return;
        s = (s + 1) & (slots - 1);
    }
}
// the walk is bounded by the table size, so that a damaged table cannot keep a lane walking
TSQ_HD bool tsq_us_set_has(const tsq_us_set& t, uint64_t handle) {
    if (t.slots == 0) return false;
    uint64_t s = tsq_us_slot(handle, t.slots);
    for (uint64_t step = 0; step < t.slots; step++) {
        if (!((t.occ[s >> 5] >> (s & 31)) & 1u)) return false;
        if (t.keys[s] == handle) return true;
        s = (s + 1) & (t.slots - 1);
    }
    return false;
}

// ---------------------------------------------------------------- the order
struct tsq_us_order {
    int32_t n_keys;
    int32_t key_col[TSQ_MAX_KEYS];
    int32_t handle_col;
    int32_t desc;
};
// One sorted input run: its columns and a view of them.  Logical row i (0 <= i < n) of the view is physical row rows[i] of the columns, or
// base + i when there is no list.
struct tsq_us_view {
    const uint32_t* rows;  // the kept-row list of the filter (snapshot side), or null
    int64_t base;          // the added-row cursor
    int64_t n;
};
struct tsq_us_run {
    tsq_colset cs;
    tsq_us_view v;
};
TSQ_HD int64_t tsq_us_phys(const tsq_us_view& r, int64_t i) { return r.rows ? (int64_t)r.rows[i] : r.base + i; }

// UnionScanExec.compare on (physical row ra of a, physical row rb of b), then inverted for desc: < 0 when a comes first in scan order
TSQ_HD int tsq_us_cmp(const tsq_us_order& o, const tsq_colset& a, int64_t ra, const tsq_colset& b, int64_t rb) {
    int c = 0;
    for (int k = 0; k < o.n_keys && c == 0; k++) {
        const int col = o.key_col[k];
        const bool na = a.nulls[col] && !((a.nulls[col][ra >> 3] >> (ra & 7)) & 1);
        const bool nb = b.nulls[col] && !((b.nulls[col][rb >> 3] >> (rb & 7)) & 1);
        if (na || nb) {  // NULL is smaller than every value; NULL and NULL: the next column decides
            c = (int)nb - (int)na;
        } else if (a.type[col] == TSQ_BYTES) {
            const int64_t la = a.offs[col][ra + 1] - a.offs[col][ra], lb = b.offs[col][rb + 1] - b.offs[col][rb];
            c = tsq_cmp_bytes((const uint8_t*)a.data[col] + a.offs[col][ra], (uint32_t)la, (const uint8_t*)b.data[col] + b.offs[col][rb], (uint32_t)lb);
        } else {
            const uint64_t ia = tsq_sort_image(a.data[col], a.type[col], 0, (uint64_t)ra), ib = tsq_sort_image(b.data[col], b.type[col], 0, (uint64_t)rb);
            c = ia < ib ? -1 : (ia > ib ? 1 : 0);
        }
    }
    if (c == 0) {  // the raw 8 bytes as a signed integer, whatever the column's type
        const int64_t ha = ((const int64_t*)a.data[o.handle_col])[ra], hb = ((const int64_t*)b.data[o.handle_col])[rb];
        c = ha < hb ? -1 : (ha > hb ? 1 : 0);
    }
    return o.desc ? -c : c;
}

// ---------------------------------------------------------------- merge path
// Output position d of merge(S, A) (0 <= d <= S.n + A.n) splits into (i, d - i): i rows of S and d - i rows of A come before it.
// Binary search of i on the diagonal; the bounds are clamped to both runs first, so that S[mid] and A[d - mid - 1] exist whatever the
// comparator answers (unsorted input gives some split, never an index outside a run).
TSQ_HD int64_t tsq_us_diag(const tsq_us_order& o, const tsq_colset& scs, const tsq_us_view& S, const tsq_colset& acs, const tsq_us_view& A, int64_t d) {
    const int64_t total = S.n + A.n;
    d = d < 0 ? 0 : (d > total ? total : d);
    int64_t lo = d - A.n > 0 ? d - A.n : 0, hi = d < S.n ? d : S.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);  // lo <= mid < hi <= min(d, S.n);  0 <= d - mid - 1 < A.n
        if (tsq_us_cmp(o, scs, tsq_us_phys(S, mid), acs, tsq_us_phys(A, d - mid - 1)) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// Step 1 -> step 2.  A TILE is the outputs [d0, d1); (i0, i1) are the splits of its two boundaries (tsq_us_diag over the whole runs).  The
// tile's outputs are the merge of S[i0, i1) and A[d0 - i0, d1 - i1): the lanes of the tile search their diagonals inside these two
// stretches only.  Every bound is clamped again here, so that splits that contradict each other (unsorted input) still give views
// that lie inside the runs; such a tile may then cover fewer outputs than d1 - d0.
TSQ_HD void tsq_us_tile_views(const tsq_us_view& S, const tsq_us_view& A, int64_t d0, int64_t d1, int64_t i0, int64_t i1, tsq_us_view* s, tsq_us_view* a) {
    const int64_t total = S.n + A.n;
    d0 = d0 < 0 ? 0 : (d0 > total ? total : d0);
    d1 = d1 < d0 ? d0 : (d1 > total ? total : d1);
    i0 = i0 < 0 ? 0 : (i0 > S.n ? S.n : i0);
    int64_t j0 = d0 - i0;
    j0 = j0 < 0 ? 0 : (j0 > A.n ? A.n : j0);
    int64_t ns = i1 - i0, cap = d1 - d0 < S.n - i0 ? d1 - d0 : S.n - i0;
    ns = ns < 0 ? 0 : (ns > cap ? cap : ns);
    int64_t na = (d1 - d0) - ns;
    na = na < 0 ? 0 : (na > A.n - j0 ? A.n - j0 : na);
    s->rows = S.rows ? S.rows + i0 : nullptr;
    s->base = S.base + i0;
    s->n = ns;
    a->rows = A.rows ? A.rows + j0 : nullptr;
    a->base = A.base + j0;
    a->n = na;
}
// A take-list entry: bit 31 = the side (0 snapshot, 1 added), bits 30:0 = the PHYSICAL row of that side.
#define TSQ_US_SIDE_ADDED 0x80000000u
// One lane's stretch: outputs [d, d + count) cut to the total, starting from the split (i, d - i); take[] is indexed by the output
// position.  Every row index is checked against its run before it is read.
TSQ_HD void tsq_us_lane_merge(const tsq_us_order& o, const tsq_colset& scs, const tsq_us_view& S, const tsq_colset& acs, const tsq_us_view& A, int64_t d, int64_t i,
                              int count, uint32_t* take) {
    const int64_t total = S.n + A.n;
    i = i < 0 ? 0 : (i > S.n ? S.n : i);
    int64_t j = d - i;
    j = j < 0 ? 0 : (j > A.n ? A.n : j);
    for (int t = 0; t < count && d + t < total; t++) {
        bool from_s;
        if (i >= S.n) from_s = false;
        else if (j >= A.n) from_s = true;
        else from_s = tsq_us_cmp(o, scs, tsq_us_phys(S, i), acs, tsq_us_phys(A, j)) < 0;
        if (!from_s && j >= A.n) break;  // (only when the clamps above moved the split: nothing left to take)
        if (from_s) take[d + t] = (uint32_t)tsq_us_phys(S, i++);
        else take[d + t] = TSQ_US_SIDE_ADDED | (uint32_t)tsq_us_phys(A, j++);
    }
}
// The streaming rule's m: how many rows of A come before physical row `last` of the snapshot columns (a lower bound in A)
TSQ_HD int64_t tsq_us_bound(const tsq_us_order& o, const tsq_colset& acs, const tsq_us_view& A, const tsq_colset& snap, int64_t last) {
    int64_t lo = 0, hi = A.n;
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (tsq_us_cmp(o, acs, tsq_us_phys(A, mid), snap, last) < 0) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}

#endif
