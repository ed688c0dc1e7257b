// tsq_compact.h — the positions pass of a selection, shared by tsq_chunk_compact (tsq_chunk.hip) and tsq_project_run (tsq_project.h):
// every WAVE owns a contiguous run of rows_per_wave rows; k_compact_count leaves the selected rows of every run, k_compact_scan (one
// workgroup) turns them into exclusive bases + the total.  The consumer walks its run in order with ballot + popcount prefix, so
// the dense rows keep the input order.  No workgroup ever waits for another one (a single-pass chained scan would: a workgroup
// spinning on a predecessor that is not resident never ends).
#ifndef TSQ_COMPACT_H
#define TSQ_COMPACT_H

#include "tsq_internal.h"

struct CompactArgs {
    tsq_colset in;
    const uint8_t* selected;  // one byte per row (Go []bool)
    int64_t nrows;
    int64_t rows_per_wave;           // rows of one wave's contiguous run (a multiple of 64)
    unsigned long long* block_base;  // per-wave counts -> exclusive bases (4 per workgroup)
    void* out_data[TSQ_MAX_COLS];
    uint8_t* out_notnull[TSQ_MAX_COLS];
    int64_t* out_offs[TSQ_MAX_COLS];  // var-len columns: the scatter leaves the cell lengths here, a scan makes them offsets
    uint32_t* src_row;                // var-len columns: source row of every dense row (for the byte copy)
    unsigned long long* total;
};

static __global__ void __launch_bounds__(256) k_compact_count(CompactArgs a) {
    const int lane = threadIdx.x & 63;
    const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // this wave's run of rows
    const int64_t lo = u * a.rows_per_wave;
    int64_t hi = lo + a.rows_per_wave;
    hi = hi < a.nrows ? hi : a.nrows;
    unsigned int c = 0;
    for (int64_t r = lo + lane; r < hi; r += 64) c += a.selected[r] ? 1u : 0u;
    for (int o = 32; o > 0; o >>= 1) c += __shfl_xor(c, o, 64);
    if (lane == 0) a.block_base[u] = c;
}
// exclusive scan of n per-workgroup counts; *total = sum
static __global__ void __launch_bounds__(1024) k_compact_scan(unsigned long long* v, int n, unsigned long long* total) {
    __shared__ unsigned long long s_w[16];
    const int per = (n + 1023) / 1024, lo = threadIdx.x * per;
    unsigned long long sum = 0;
    for (int i = lo; i < lo + per && i < n; i++) sum += v[i];
    unsigned long long x = sum;
    for (int o = 1; o < 64; o <<= 1) {
        const unsigned long long y = __shfl_up(x, o, 64);
        if ((int)(threadIdx.x & 63) >= o) x += y;
    }
    if ((threadIdx.x & 63) == 63) s_w[threadIdx.x >> 6] = x;
    __syncthreads();
    unsigned long long pre = 0, all = 0;
    for (int w = 0; w < 16; w++) {
        if (w < (int)(threadIdx.x >> 6)) pre += s_w[w];
        all += s_w[w];
    }
    unsigned long long run = pre + x - sum;
    for (int i = lo; i < lo + per && i < n; i++) {
        const unsigned long long c = v[i];
        v[i] = run;
        run += c;
    }
    if (threadIdx.x == 0) *total = all;
}

#endif
