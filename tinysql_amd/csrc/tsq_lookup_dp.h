// tsq_lookup_dp.h — the scalar core of the IndexLookUp handle search (tsq_lookup.hip): the shape of the sampled search index over a
// table's ascending handles, the lower bound inside one level and the descent from the top level to the table.
// TSQ_HD so that the CPU test-suite compiles the very same code on the host, sanitized (tests/lookup_dp_main.cpp): an index that
// leaves its level is found there, not on the GPU.
// Reference: the table worker of IndexLookUpExecutor reads the rows of a task's handles by point ranges
// (executor/distsql.go:558-637, distsql/request_builder.go:161-180); the order of record keys is the order of EncodeInt(handle),
// i.e. handles as SIGNED int64 (tablecodec/tablecodec.go:65-70).
//
// Level 0 is the table (n[0] handles, strictly ascending).  Level k + 1 holds every 2^shift-th entry of level k, from its first one:
// lv[k + 1][j] = lv[k][j << shift], n[k + 1] = ceil(n[k] / 2^shift).  Levels are added while the top one has more than
// TSQ_LK_TOP_MAX entries (what the search kernel stages in LDS), at most TSQ_LK_MAX_LEVELS of them; shift = 0: no level, the plain
// lower bound over the whole table.
// Every index below is bounded by the n[] of the plan alone, never by the data: tables that are not ascending give a wrong
// position, not a read outside a level (tsq_lookup_create refuses them anyway).
#ifndef TSQ_LOOKUP_DP_H
#define TSQ_LOOKUP_DP_H

#include "tsq_device.h"

#define TSQ_LK_MAX_LEVELS 8
#define TSQ_LK_TOP_MAX 1024
#define TSQ_LK_MAX_SHIFT 16

struct tsq_lk_index {
    const int64_t* lv[TSQ_LK_MAX_LEVELS + 1];  // lv[0] = the table's handles
    int64_t n[TSQ_LK_MAX_LEVELS + 1];
    int32_t levels;  // sampled levels above the table
    int32_t shift;
};

// fills n[1..] and levels from n[0] = n_rows; returns the number of sampled levels
TSQ_HD int tsq_lk_plan(tsq_lk_index* ix, int64_t n_rows, int shift, int64_t top_max) {
    ix->n[0] = n_rows < 0 ? 0 : n_rows;
    ix->shift = shift < 0 ? 0 : (shift > TSQ_LK_MAX_SHIFT ? TSQ_LK_MAX_SHIFT : shift);
    ix->levels = 0;
    for (int k = 1; k <= TSQ_LK_MAX_LEVELS; k++) ix->n[k] = 0;
    if (ix->shift == 0) return 0;
    while (ix->levels < TSQ_LK_MAX_LEVELS && ix->n[ix->levels] > top_max) {
        const int64_t below = ix->n[ix->levels];
        ix->n[ix->levels + 1] = ((below - 1) >> ix->shift) + 1;
        ix->levels++;
    }
    return ix->levels;
}
// entry of the level below that becomes entry j of a sampled level
TSQ_HD int64_t tsq_lk_sample_src(int64_t j, int shift) { return j << shift; }

// first i in [lo, hi) with a[i] >= x as signed int64, hi when there is none
TSQ_HD int64_t tsq_lk_lower(const int64_t* a, int64_t lo, int64_t hi, int64_t x) {
    while (lo < hi) {
        const int64_t mid = lo + ((hi - lo) >> 1);
        if (a[mid] < x) lo = mid + 1;
        else hi = mid;
    }
    return lo;
}
// c = the lower bound of x in level `from`: entry c - 1 of that level is < x and entry c (if there is one) is >= x.  One level down
// these are entries (c - 1) << shift and c << shift, so the lower bound there lies in ((c - 1) << shift, c << shift]: at most
// 2^shift - 1 entries to search, `shift` steps.
TSQ_HD int64_t tsq_lk_descend(const tsq_lk_index& ix, int from, int64_t c, int64_t x) {
    for (int k = from; k > 0; k--) {
        const int64_t nb = ix.n[k - 1];
        int64_t lo = c > 0 ? ((c - 1) << ix.shift) + 1 : 0;
        int64_t hi = c << ix.shift;
        hi = hi < nb ? hi : nb;
        lo = lo < hi ? lo : hi;
        c = tsq_lk_lower(ix.lv[k - 1], lo, hi, x);
    }
    return c;
}
// the lower bound of x in the table; `top` = the top level (ix.lv[ix.levels], or a copy of it in faster memory)
TSQ_HD int64_t tsq_lk_search(const tsq_lk_index& ix, const int64_t* top, int64_t x) {
    return tsq_lk_descend(ix, ix.levels, tsq_lk_lower(top, 0, ix.n[ix.levels], x), x);
}
// the row of handle x, or -1
TSQ_HD int64_t tsq_lk_find(const tsq_lk_index& ix, const int64_t* top, int64_t x) {
    const int64_t p = tsq_lk_search(ix, top, x);
    return p < ix.n[0] && ix.lv[0][p] == x ? p : -1;
}

// tsq_lookup.hip, for the other units of the library: the handle's copy of the table's handles and the search index over it
struct tsq_lookup;
const tsq_lk_index* tsq_lookup_index_of(const tsq_lookup* l);

// the arguments of the gather kernels (tsq_rows_gather, K18e / K18f)
struct RgArgs {
    const uint8_t* values;
    int64_t n_bytes;
    const int64_t* offsets;  // [n_src_rows + 1]
    int64_t n_src_rows;
    const int64_t* rows;     // [n]
    int64_t n;
    int64_t* lens;           // [n + 1]: lengths, then (scan) output offsets
    unsigned int* err;       // bit 0: a row index out of range; bit 1: an offset pair that decreases or leaves the values
    uint8_t* out;
    int64_t* out_offsets;    // [n + 1]
    int64_t wave_copy;       // rows of at least this many bytes are copied by the wave; <= 0: never
};
// K18f alone on the context's stream: lens already holds the n + 1 output offsets, rows and offsets were checked by the caller
struct tsq_ctx;
struct tsq_handle_hdr;
tsq_status tsq_launch_rg_copy(tsq_ctx* ctx, tsq_handle_hdr* h, const RgArgs& a);

#endif
