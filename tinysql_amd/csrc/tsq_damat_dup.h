// tsq_damat_dup.h — the materialising packed join with the build side in LDS, DUPLICATE build keys (round 9; device code, included by
// tsq_join.hip).
//
// tsq_damat.h keeps a final partition's build rows in a ranked LDS table, but only for a build side without duplicate keys: there a probe
// row makes exactly one output row and its place is its index.  A build side with duplicate keys (any FK-FK join, any join whose build side
// is the "many" side; the reference's own join tests: executor/join_test.go:101-104, 134-160) went to the sorted-build-columns variant
// (k_da_emit_cols), one random 8-byte HBM read per build cell.  The byte cells of the images bound the multiplicity at 255 (da_prepare
// hands anything beyond to the 64-bit route), so a final partition's build rows still fit in LDS; what changes is that one probe row
// makes up to 255 output rows.  Levels 1 and 2 (k_da_partition_cols, k_dm_split) are those of tsq_damat.h, unchanged, for both sides;
// the bitmap an inner join's level 2 filters with is "cell != 0" (k_dmd_bytes_to_bits).
//   table    per final partition: presence bits + popcount prefix per 32 cells (as k_dm_emit), start[d] for every distinct key
//            d = rank_of(e) (start[D] = the partition's build rows), and the payload cells + NOT-NULL bits of the build rows in RUN order:
//            a counting sort by cell in LDS (count per d, exclusive scan, scatter with a per-d cursor; the order inside a run is free, as in
//            the reference).  The sort is redone by every launch — no second copy of the build side in HBM, no second preparation kernel;
//            it touches 2 + 8 x columns bytes per build row, what a straight copy of a sorted partition would read as well
//   count    k_dmd_count: one workgroup per final partition, the build rows per distinct key in LDS (the lengths of the runs: no scan, no
//            payload), the probe entries stream at 2 B each -> the OUTPUT rows of the partition, in an array of their own (the emit
//            kernel still needs the probe ROWS k_dm_split left in pst.cnt); k_dm_scan turns them into output bases
//   emit     k_dmd_emit: the probe rows in tiles; a block-wide exclusive scan of the tile's multiplicities, then the writes are assigned by
//            OUTPUT row: a lane owns two consecutive output rows, finds its probe row by binary search over the scanned offsets and its
//            place in the run by subtraction — every column is written as contiguous rows by consecutive lanes whatever the
//            multiplicities (16-byte non-temporal stores on 16-byte boundaries)
// Replaces (reference): joiner.tryToMatchInners / onMissMatch + Chunk.AppendRow (joiner.go:145-410, chunk.go:334-356).
// Bytes per unit: count 2 per build row + 2 per probe row; emit 2 + 8 x build columns per build row, 2 + 8 x travelling columns per probe
// row (re-read from L2 by the output rows of one probe row), 8 per output cell + 1 per nullable output cell written.
#ifndef TSQ_DAMAT_DUP_H
#define TSQ_DAMAT_DUP_H

#include "tsq_damat.h"

struct DmdCountArgs {
    DmStore bst, pst;                   // final partitions of the build / the probe side (pst.cnt: probe ROWS per partition, not scanned)
    uint32_t pbits;                     // log2 of the final partitions
    uint32_t tab_rows;                  // >= the build rows of the largest final partition
    unsigned long long* out_rows;       // [Q + 1] output rows per final partition (k_dm_scan makes bases of them)
};
struct DmdEmitArgs {
    DmEmitArgs e;                       // as k_dm_emit's; e.pst.cnt holds the probe ROWS per partition
    const unsigned long long* obase;    // [Q + 1] scanned output rows per final partition
    uint8_t* out_head;                  // (null: not wanted) 1: this output row is the first of its probe row's candidates
};

// LDS of k_dmd_count: presence bits | popcount prefix | build rows per distinct key
__host__ __device__ inline size_t dmd_count_lds(uint32_t ebits2, uint32_t tab_rows) {
    const size_t words = ((size_t)1 << ebits2) / 32 + 1;
    return words * 8 + ((size_t)tab_rows + 2) * 4 + 16;
}
// LDS of k_dmd_emit<NT>: presence bits | popcount prefix | n_build payload tables | their NOT-NULL bits | start[] | per tile of 2 NT probe
// rows: the scanned offsets, the rows' run starts, the rows' entries
__host__ __device__ inline size_t dmd_emit_lds(uint32_t ebits2, uint32_t tab_rows, int n_build, bool build_nulls, uint32_t nt) {
    const size_t words = ((size_t)1 << ebits2) / 32 + 1;
    const size_t tile = (size_t)nt * 2;
    return words * 8 + (size_t)tab_rows * 8 * (size_t)(n_build > 0 ? n_build : 0) + (build_nulls ? (size_t)n_build * (tab_rows / 8) : 0) + ((size_t)tab_rows + 2) * 4 +
           (tile + 1) * 4 + tile * 4 + tile * 2 + 32;
}

// byte cells (the build rows of every key of the domain, <= 255) -> one bit per cell: cell != 0.  What level 2 filters an inner join's probe
// rows with (k_da_bytes_to_bits takes bit 0 of a byte: right for the cells 0 / 1 of a unique build side only)
static __global__ void __launch_bounds__(256) k_dmd_bytes_to_bits(const uint8_t* img, uint32_t* bits, size_t nwords) {
    for (size_t i = (size_t)blockIdx.x * 256 + threadIdx.x; i < nwords; i += (size_t)gridDim.x * 256) {
        const uint4* b = reinterpret_cast<const uint4*>(img + i * 32);
        const uint4 x = b[0], y = b[1];
        const uint32_t w[8] = {x.x, x.y, x.z, x.w, y.x, y.y, y.z, y.w};
        uint32_t out = 0;
#pragma unroll
        for (uint32_t k = 0; k < 8; k++) {
            const uint32_t v = ((w[k] | ((w[k] & 0x7f7f7f7fu) + 0x7f7f7f7fu)) >> 7) & 0x01010101u;  // byte != 0 -> its bit 0
            out |= (((v * 0x10204080u) >> 28) & 0xfu) << (k * 4u);
        }
        bits[i] = out;
    }
}

// presence bits and popcount prefix of a final partition's build rows (as k_dm_emit; ends with the table visible to every thread)
template <int NT>
__device__ __forceinline__ void dmd_bits_and_prefix(const uint16_t* bent, uint32_t bcnt, uint32_t W, uint32_t* s_bits, uint32_t* s_coarse, uint32_t* s_wsum) {
    const uint32_t tid = threadIdx.x, wpt = (W + NT - 1) / NT;
    for (uint32_t i = tid; i < W; i += NT) s_bits[i] = 0;
    __syncthreads();
    const uint4* eb = reinterpret_cast<const uint4*>(bent);
    for (uint32_t x = tid; x < (bcnt + 7u) >> 3; x += NT) {
        const uint4 ev = eb[x];
        const uint32_t ew[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
        for (uint32_t i = 0; i < 8; i++) {
            const uint32_t e = (ew[i >> 1] >> ((i & 1u) * 16u)) & 0xffffu;
            if (x * 8u + i < bcnt) atomicOr(&s_bits[e >> 5], 1u << (e & 31u));
        }
    }
    __syncthreads();
    uint32_t sum = 0;
    for (uint32_t k = 0; k < wpt; k++) {
        const uint32_t w = tid * wpt + k;
        sum += w < W ? (uint32_t)__popc(s_bits[w]) : 0u;
    }
    uint32_t total;
    uint32_t run = block_excl_scan<NT>(sum, s_wsum, &total);
    for (uint32_t k = 0; k < wpt; k++) {
        const uint32_t w = tid * wpt + k;
        if (w < W) {
            s_coarse[w] = run;
            run += (uint32_t)__popc(s_bits[w]);
        }
    }
    __syncthreads();
}

template <int NT, bool OUTER>
__global__ void __launch_bounds__(NT) k_dmd_count(DmdCountArgs a) {
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ uint32_t s_wsum[NT / 64];
    __shared__ unsigned long long s_total;
    const uint32_t tid = threadIdx.x;
    const uint32_t Q = 1u << a.pbits, cells = 1u << a.pst.ebits2, W = cells >= 32u ? cells / 32u : 1u;
    uint32_t* s_bits = reinterpret_cast<uint32_t*>(s_dyn);
    uint32_t* s_coarse = s_bits + W;
    uint32_t* s_m = s_coarse + W;       // [tab_rows + 1] build rows of distinct key d
    for (uint32_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const uint32_t bcnt = (uint32_t)a.bst.cnt[q], boff = a.bst.off[q];
        const uint32_t pcnt = (uint32_t)a.pst.cnt[q], poff = a.pst.off[q];
        if (pcnt == 0) {  // (block-uniform)
            if (tid == 0) a.out_rows[q] = 0;
            continue;
        }
        __syncthreads();  // the previous partition's probe rows are done with the table
        for (uint32_t i = tid; i <= a.tab_rows; i += NT) s_m[i] = 0;
        if (tid == 0) s_total = 0;
        dmd_bits_and_prefix<NT>(a.bst.ent + boff, bcnt, W, s_bits, s_coarse, s_wsum);
        auto rank_of = [&](uint32_t e) -> uint32_t { return s_coarse[e >> 5] + (uint32_t)__popc(s_bits[e >> 5] & ((1u << (e & 31u)) - 1u)); };
        for (uint32_t i = tid; i < bcnt; i += NT) atomicAdd(&s_m[rank_of(a.bst.ent[boff + i])], 1u);
        __syncthreads();
        // ---- the probe entries (units of 8: a final partition starts on a multiple of 8 slots)
        unsigned long long sum = 0;
        const uint4* pe = reinterpret_cast<const uint4*>(a.pst.ent + poff);
        for (uint32_t x = tid; x < (pcnt + 7u) >> 3; x += NT) {
            const uint4 ev = pe[x];
            const uint32_t ew[4] = {ev.x, ev.y, ev.z, ev.w};
#pragma unroll
            for (uint32_t i = 0; i < 8; i++) {
                const uint32_t e = (ew[i >> 1] >> ((i & 1u) * 16u)) & 0xffffu;
                if (x * 8u + i < pcnt) {
                    const bool has = (s_bits[e >> 5] >> (e & 31u)) & 1u;
                    const uint32_t m = has ? s_m[rank_of(e)] : 0u;
                    sum += OUTER ? (m ? m : 1u) : m;
                }
            }
        }
        sum = wave_sum_u64(sum);
        if ((tid & 63u) == 0 && sum) atomicAdd(&s_total, sum);
        __syncthreads();
        if (tid == 0) a.out_rows[q] = s_total;
    }
}

template <int NT, bool OUTER>
__global__ void __launch_bounds__(NT) k_dmd_emit(DmdEmitArgs da) {
    constexpr uint32_t TP = NT * 2;     // probe rows per tile
    const DmEmitArgs& a = da.e;
    extern __shared__ __align__(16) unsigned char s_dyn[];
    __shared__ uint32_t s_wsum[NT / 64];
    const uint32_t tid = threadIdx.x;
    const uint32_t Q = 1u << a.pbits, ebits2 = a.pst.ebits2, cells = 1u << ebits2, W = cells >= 32u ? cells / 32u : 1u;
    const int nb = a.n_build > 0 ? a.n_build : 0;
    const bool bnulls = a.bst.nnmask != nullptr;
    const uint32_t nnw = a.tab_rows / 32u;  // NOT-NULL words per build column
    uint32_t* s_bits = reinterpret_cast<uint32_t*>(s_dyn);
    uint32_t* s_coarse = s_bits + W;
    uint64_t* s_tab = reinterpret_cast<uint64_t*>(s_dyn + (((size_t)W * 8 + 15) & ~(size_t)15));
    uint32_t* s_tnn = reinterpret_cast<uint32_t*>(s_tab + (size_t)a.tab_rows * (size_t)nb);
    uint32_t* s_start = s_tnn + (bnulls ? nnw * (uint32_t)nb : 0u);  // [tab_rows + 2]
    uint32_t* s_off = s_start + a.tab_rows + 2;                      // [TP + 1] output rows of the tile before probe row i
    uint32_t* s_st = s_off + TP + 1;                                 // [TP] start[d] of probe row i's run (~0: no build row)
    uint16_t* s_e = reinterpret_cast<uint16_t*>(s_st + TP);          // [TP] the rows' entries
    for (uint32_t q = blockIdx.x; q < Q; q += gridDim.x) {
        const uint32_t bcnt = (uint32_t)a.bst.cnt[q], boff = a.bst.off[q];
        const uint32_t pcnt = (uint32_t)a.pst.cnt[q], poff = a.pst.off[q];
        const unsigned long long ob0 = da.obase[q];
        if (da.obase[q + 1] == ob0) continue;  // (block-uniform) no output row: no probe row, or none with a build row
        __syncthreads();  // the previous partition's probe rows are done with the table
        for (uint32_t i = tid; i < a.tab_rows + 2; i += NT) s_start[i] = 0;
        if (bnulls)
            for (uint32_t i = tid; i < nnw * (uint32_t)nb; i += NT) s_tnn[i] = 0xffffffffu;
        dmd_bits_and_prefix<NT>(a.bst.ent + boff, bcnt, W, s_bits, s_coarse, s_wsum);
        auto rank_of = [&](uint32_t e) -> uint32_t { return s_coarse[e >> 5] + (uint32_t)__popc(s_bits[e >> 5] & ((1u << (e & 31u)) - 1u)); };
        // ---- the runs: the rows of distinct key d are counted at s_start[d + 2]; an inclusive scan then leaves start[d] at s_start[d + 1],
        // which is the cursor the scatter advances — to start[d + 1].  Afterwards s_start[d] = start[d] for every d (s_start[0] = 0)
        for (uint32_t i = tid; i < bcnt; i += NT) atomicAdd(&s_start[rank_of(a.bst.ent[boff + i]) + 2u], 1u);
        __syncthreads();
        {
            const uint32_t n = a.tab_rows + 2, per = (n + NT - 1) / NT, lo = tid * per;
            uint32_t sum = 0;
            for (uint32_t i = lo; i < lo + per && i < n; i++) sum += s_start[i];
            uint32_t total;
            uint32_t run = block_excl_scan<NT>(sum, s_wsum, &total);
            for (uint32_t i = lo; i < lo + per && i < n; i++) {
                run += s_start[i];
                s_start[i] = run;
            }
        }
        __syncthreads();
        // (now s_start[d + 1] = start[d], s_start[d + 2] = start[d + 1])
        {
            for (uint32_t x = tid; x < (bcnt + 1u) >> 1; x += NT) {
                const uint32_t ew = *reinterpret_cast<const uint32_t*>(a.bst.ent + boff + (size_t)x * 2u);
                const bool v1 = x * 2u + 1u < bcnt;
                const uint32_t r0 = atomicAdd(&s_start[rank_of(ew & 0xffffu) + 1u], 1u);
                const uint32_t r1 = v1 ? atomicAdd(&s_start[rank_of(ew >> 16) + 1u], 1u) : 0u;
                for (int v = 0; v < nb; v++) {
                    const ulonglong2 c = *reinterpret_cast<const ulonglong2*>(a.bst.pay[v] + boff + (size_t)x * 2u);
                    s_tab[(size_t)v * a.tab_rows + r0] = c.x;
                    if (v1) s_tab[(size_t)v * a.tab_rows + r1] = c.y;
                }
                if (bnulls) {
                    const uint32_t m = *reinterpret_cast<const uint16_t*>(a.bst.nnmask + boff + (size_t)x * 2u);
                    for (int v = 0; v < nb; v++) {
                        if (!((m >> v) & 1u)) atomicAnd(&s_tnn[(uint32_t)v * nnw + (r0 >> 5)], ~(1u << (r0 & 31u)));
                        if (v1 && !((m >> (8 + v)) & 1u)) atomicAnd(&s_tnn[(uint32_t)v * nnw + (r1 >> 5)], ~(1u << (r1 & 31u)));
                    }
                }
            }
        }
        __syncthreads();
        // (now run d = [s_start[d], s_start[d + 1]): the cursor of d ended at start[d + 1], s_start[0] = 0)
        // ---- the probe rows, TP per tile
        unsigned long long tbase = a.row0 + ob0;  // first output row of the tile
        const uint16_t* pe = a.pst.ent + poff;
        for (uint32_t t0 = 0; t0 < pcnt; t0 += TP) {
            const uint32_t rows = pcnt - t0 < TP ? pcnt - t0 : TP;
            __syncthreads();  // the previous tile's output rows are done with the tile arrays
            uint32_t m0 = 0, m1 = 0;
            {
                const uint32_t i0 = tid * 2u;  // a thread scans two neighbouring probe rows (one 4-byte load of entries)
                if (i0 < rows) {
                    const uint32_t ew = *reinterpret_cast<const uint32_t*>(pe + t0 + i0);
                    const uint32_t e0 = ew & 0xffffu, e1 = ew >> 16;
                    const bool h0 = (s_bits[e0 >> 5] >> (e0 & 31u)) & 1u, h1 = i0 + 1u < rows && ((s_bits[e1 >> 5] >> (e1 & 31u)) & 1u);
                    uint32_t st0 = ~0u, st1 = ~0u;
                    if (h0) {
                        const uint32_t d = rank_of(e0);
                        st0 = s_start[d];
                        m0 = s_start[d + 1] - st0;
                    }
                    if (h1) {
                        const uint32_t d = rank_of(e1);
                        st1 = s_start[d];
                        m1 = s_start[d + 1] - st1;
                    }
                    if (OUTER) {
                        m0 = m0 ? m0 : 1u;
                        m1 = i0 + 1u < rows ? (m1 ? m1 : 1u) : 0u;
                    }
                    s_st[i0] = st0;
                    s_st[i0 + 1] = st1;
                    s_e[i0] = (uint16_t)e0;
                    s_e[i0 + 1] = (uint16_t)e1;
                }
            }
            uint32_t tile_out;
            const uint32_t ex = block_excl_scan<NT>(m0 + m1, s_wsum, &tile_out);
            if (tid * 2u < rows) {
                s_off[tid * 2u] = ex;
                s_off[tid * 2u + 1] = ex + m0;
            }
            if (tid == 0) s_off[rows] = tile_out;  // (rows odd: the second row of the last pair has m = 0 and wrote the same value)
            __syncthreads();
            // ---- by OUTPUT row: lane x owns the two rows that share a 16-byte unit of the output columns (an odd base shifts the pairing)
            const uint32_t sh = (uint32_t)tbase & 1u;
            const uint32_t npairs = (tile_out + sh + 1u) >> 1;
            for (uint32_t x = tid; x < npairs; x += NT) {
                const int64_t t = (int64_t)x * 2 - (int64_t)sh;  // rows t, t + 1 of the tile's output
                const bool v0 = t >= 0, v1 = t + 1 < (int64_t)tile_out;
                // the probe row of the first valid row: the last i with s_off[i] <= its t (rows with m = 0 share their successor's offset: skipped)
                const uint32_t tf = v0 ? (uint32_t)t : (uint32_t)(t + 1);
                uint32_t lo = 0, hi = rows;  // s_off[lo] <= tf < s_off[hi]
                while (hi - lo > 1u) {
                    const uint32_t mid = (lo + hi) >> 1;
                    if (s_off[mid] <= tf) lo = mid;
                    else hi = mid;
                }
                uint32_t ia = lo, ka = tf - s_off[lo];
                uint32_t ib = ia, kb = ka;
                if (v0 && v1) {  // the second row: the next of the run, or the first of the next probe row that has output rows
                    kb = ka + 1u;
                    if ((uint32_t)t + 1u >= s_off[ia + 1]) {
                        ib = ia + 1u;
                        while (s_off[ib + 1] <= (uint32_t)t + 1u) ib++;
                        kb = 0;
                    }
                }
                const uint32_t sta = s_st[ia], stb = s_st[ib];
                const bool ha = sta != ~0u, hb = stb != ~0u;  // (an inner join's rows all have build rows)
                const uint32_t ra = ha ? sta + ka : 0u, rb = hb ? stb + kb : 0u;
                const unsigned long long g = tbase + (unsigned long long)t;
                auto put = [&](uint64_t* col, uint64_t c0, uint64_t c1) {
                    if (v0 && v1) {
                        tsq_v2u64 y;
                        y.x = c0;
                        y.y = c1;
                        __builtin_nontemporal_store(y, reinterpret_cast<tsq_v2u64*>(col + g));
                    } else if (v0) TSQ_EMIT_STORE(&col[g], c0);
                    else if (v1) TSQ_EMIT_STORE(&col[g + 1], c1);
                };
                // NOT-NULL byte flags: EVERY row's flag is written — the arrays arrive uninitialised (see k_dm_emit)
                auto put_null = [&](uint8_t* nn, bool n0, bool n1) {
                    if (v0 && v1) *reinterpret_cast<uint16_t*>(nn + g) = (uint16_t)((n0 ? 0u : 1u) | (n1 ? 0u : 0x100u));
                    else if (v0) nn[g] = n0 ? 0 : 1;
                    else if (v1) nn[g + 1] = n1 ? 0 : 1;
                };
                // (a lane with one valid row has ia = ib, ka = kb: both halves name that row)
                const size_t pa = (size_t)poff + t0 + ia, pb = (size_t)poff + t0 + ib;
                uint32_t mma = 0xffu, mmb = 0xffu;
                if (a.pst.nnmask) {
                    mma = a.pst.nnmask[pa];
                    mmb = a.pst.nnmask[pb];
                }
                for (int v = 0; v < a.n_probe; v++) {
                    const uint64_t* src = a.pst.pay[v];
                    put(a.out_probe[v], src[pa], src[pb]);
                    if (a.out_probe_nn[v]) put_null(a.out_probe_nn[v], !((mma >> v) & 1u), !((mmb >> v) & 1u));
                }
                if (a.out_pkey) {
                    const uint64_t k0 = a.dm.kmin + (uint64_t)tsq_da_unmix((q << ebits2) | (uint32_t)s_e[ia], a.dm.s, a.dm.mask);
                    const uint64_t k1 = a.dm.kmin + (uint64_t)tsq_da_unmix((q << ebits2) | (uint32_t)s_e[ib], a.dm.s, a.dm.mask);
                    put(a.out_pkey, k0, k1);
                    put(a.out_bkey, (!OUTER || ha) ? k0 : 0ull, (!OUTER || hb) ? k1 : 0ull);
                    if (a.out_pkey_nn) put_null(a.out_pkey_nn, false, false);
                    if (a.out_bkey_nn) put_null(a.out_bkey_nn, OUTER && !ha, OUTER && !hb);
                }
                for (int v = 0; v < nb; v++) {
                    const uint64_t* tab = s_tab + (size_t)v * a.tab_rows;
                    put(a.out_build[v], ha ? tab[ra] : 0ull, hb ? tab[rb] : 0ull);
                    if (a.out_build_nn[v]) {
                        const uint32_t* tn = s_tnn + (uint32_t)v * nnw;
                        put_null(a.out_build_nn[v], !ha || (bnulls && !((tn[ra >> 5] >> (ra & 31u)) & 1u)), !hb || (bnulls && !((tn[rb >> 5] >> (rb & 31u)) & 1u)));
                    }
                }
                if (da.out_head) {
                    if (v0) da.out_head[g] = ka == 0 ? 1 : 0;
                    if (v1) da.out_head[g + 1] = kb == 0 ? 1 : 0;
                }
            }
            tbase += tile_out;
        }
    }
}

#endif
