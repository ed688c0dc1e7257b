// tools/interval_ubench.hip — k_da_interval_count (csrc/tsq_dajoin.h: COUNT(*) against a build side that fills its key interval) next to a
// read-and-sum kernel with the same load shape, over the same 1e8-key column: workgroup size x workgroups per CU arms, and an odd
// (8-byte aligned only) column start.  Every arm: `reps` launches of each kernel, alternating, HIP events around each launch; median [min .. max].
// The interval kernel's count is checked against the host's in every arm.  Results: profiles/r15_interval_ab.txt.
// build: hipcc --offload-arch=gfx950 -O3 -std=c++17 -mllvm -amdgpu-atomic-optimizer-strategy=None -I tinysql_amd/csrc -I include tools/interval_ubench.hip -o tools/interval_ubench
#include <hip/hip_runtime.h>
#include <algorithm>
#include <cstdio>
#include <cstring>
#include <vector>
#include "tsq_dajoin.h"

#define CK(x) do { hipError_t e_ = (x); if (e_ != hipSuccess) { printf("HIP error %s at %s:%d\n", hipGetErrorString(e_), __FILE__, __LINE__); return 2; } } while (0)

// the same tiles, the same four non-temporal 16-byte loads per lane, the same end (wave sum, one LDS add per wave, one device atomic per workgroup);
// the sum of the cells instead of the range test
template <int NT>
__global__ void __launch_bounds__(NT) k_read_sum(DaSrc src, unsigned long long* out) {
    constexpr int U = 4;
    constexpr int64_t TU = (int64_t)NT * U;
    __shared__ unsigned long long s_total;
    const uint32_t tid = threadIdx.x;
    if (tid == 0) s_total = 0;
    __syncthreads();
    const int64_t n = src.nrows;
    const int64_t head = (n > 0 && (reinterpret_cast<uintptr_t>(src.data) & 8u)) ? 1 : 0;
    const int64_t nunits = (n - head) >> 1;
    const tsq_v2u64* const col = reinterpret_cast<const tsq_v2u64*>(src.data + head);
    uint64_t sum = 0;
    const int64_t ntiles = nunits / TU;
    for (int64_t t = blockIdx.x; t < ntiles; t += gridDim.x) {
        const int64_t q0 = t * TU + tid;
        tsq_v2u64 v[U];
#pragma unroll
        for (int x = 0; x < U; x++) v[x] = __builtin_nontemporal_load(col + q0 + x * NT);
#pragma unroll
        for (int x = 0; x < U; x++) sum += v[x].x + v[x].y;
    }
    for (int64_t q = ntiles * TU + (int64_t)blockIdx.x * NT + tid; q < nunits; q += (int64_t)gridDim.x * NT) {
        const tsq_v2u64 v = __builtin_nontemporal_load(col + q);
        sum += v.x + v.y;
    }
    if (blockIdx.x == 0 && tid == 0 && head) sum += src.data[0];
    if (blockIdx.x == 0 && tid == 1 && ((n - head) & 1)) sum += src.data[n - 1];
    sum = wave_sum_u64(sum);
    if ((tid & 63u) == 0 && sum) atomicAdd(&s_total, (unsigned long long)sum);
    __syncthreads();
    if (tid == 0 && s_total) atomicAdd(&out[0], s_total);
}

struct Times {
    float med, lo, hi;
};
static Times summarise(std::vector<float> v) {
    std::sort(v.begin(), v.end());
    return Times{v[v.size() / 2], v.front(), v.back()};
}

template <int NT>
static int arm(const DaSrc& src, const DaDomain& dm, unsigned long long* dout, int cus, int per_cu, int reps, uint64_t want_count, uint64_t want_sum, const char* note) {
    const int64_t tiles = (src.nrows / 2 + NT * 4 - 1) / (NT * 4);
    const unsigned grid = (unsigned)std::max<int64_t>(1, std::min<int64_t>(tiles, (int64_t)cus * per_cu));
    hipEvent_t e0, e1;
    CK(hipEventCreate(&e0));
    CK(hipEventCreate(&e1));
    std::vector<float> ti, tr;
    unsigned long long got[2];
    for (int rep = -3; rep < reps; rep++) {  // three warm-up rounds
        for (int which = 0; which < 2; which++) {
            CK(hipMemsetAsync(dout, 0, 16, 0));
            CK(hipEventRecord(e0, 0));
            if (which == 0) hipLaunchKernelGGL((k_da_interval_count<NT, false>), dim3(grid), dim3(NT), 0, 0, src, dm, dout);
            else hipLaunchKernelGGL((k_read_sum<NT>), dim3(grid), dim3(NT), 0, 0, src, dout + 1);
            CK(hipGetLastError());
            CK(hipEventRecord(e1, 0));
            CK(hipEventSynchronize(e1));
            float ms;
            CK(hipEventElapsedTime(&ms, e0, e1));
            CK(hipMemcpy(got, dout, 16, hipMemcpyDeviceToHost));
            if (which == 0 && got[0] != want_count) { printf("WRONG COUNT %llu != %llu (NT %d, %d per CU)\n", got[0], (unsigned long long)want_count, NT, per_cu); return 1; }
            if (which == 1 && got[1] != want_sum) { printf("WRONG SUM (NT %d, %d per CU)\n", NT, per_cu); return 1; }
            if (rep >= 0) (which == 0 ? ti : tr).push_back(ms);
        }
    }
    const Times a = summarise(ti), b = summarise(tr);
    const double gb = 8.0 * (double)src.nrows / 1e9;
    printf("NT %4d x %d per CU (grid %5u)%s: interval %.4f ms [%.4f .. %.4f] %.2f TB/s | read-and-sum %.4f ms [%.4f .. %.4f] %.2f TB/s\n", NT, per_cu, grid, note, a.med, a.lo, a.hi,
           gb / a.med, b.med, b.lo, b.hi, gb / b.med);
    CK(hipEventDestroy(e0));
    CK(hipEventDestroy(e1));
    return 0;
}

int main(int argc, char** argv) {
    const int64_t n = argc > 1 ? atoll(argv[1]) : 100000000LL;
    const int reps = argc > 2 ? atoi(argv[2]) : 20;
    hipDeviceProp_t prop;
    CK(hipGetDeviceProperties(&prop, 0));
    const int cus = prop.multiProcessorCount;
    // the headline's probe column: keys of [0, 2n) in a scrambled order, half of them inside the build side's interval [0, n)
    std::vector<uint64_t> keys((size_t)n + 1);
    uint64_t want_count[2] = {0, 0}, want_sum[2] = {0, 0};
    for (int64_t i = 0; i <= n; i++) keys[(size_t)i] = ((uint64_t)i * 0x9E3779B97F4A7C15ull >> 20) % (uint64_t)(2 * n);
    for (int64_t i = 0; i <= n; i++) {
        const uint64_t k = keys[(size_t)i];
        if (i < n) { want_count[0] += k < (uint64_t)n; want_sum[0] += k; }
        if (i > 0) { want_count[1] += k < (uint64_t)n; want_sum[1] += k; }
    }
    uint64_t* dkeys;
    unsigned long long* dout;
    CK(hipMalloc(&dkeys, ((size_t)n + 1) * 8 + 64));
    CK(hipMalloc(&dout, 16));
    CK(hipMemcpy(dkeys, keys.data(), ((size_t)n + 1) * 8, hipMemcpyHostToDevice));
    const DaDomain dm{0, (uint64_t)n - 1, 27, 14, (1u << 27) - 1, 0};
    printf("%lld keys, %d CUs, %d launches of each kernel per arm (alternating), median [min .. max]\n", (long long)n, cus, reps);
    for (int off = 0; off < 2; off++) {
        DaSrc src;
        memset(&src, 0, sizeof src);
        src.data = dkeys + off;  // off = 1: the column starts on an odd cell (head row peeled, last row alone)
        src.nrows = n;
        const char* note = off ? ", odd start" : "";
        int rc = 0;
        if (off == 0) {
            rc = rc ? rc : arm<256>(src, dm, dout, cus, 2, reps, want_count[off], want_sum[off], note);
            rc = rc ? rc : arm<256>(src, dm, dout, cus, 4, reps, want_count[off], want_sum[off], note);
            rc = rc ? rc : arm<256>(src, dm, dout, cus, 8, reps, want_count[off], want_sum[off], note);
            rc = rc ? rc : arm<512>(src, dm, dout, cus, 2, reps, want_count[off], want_sum[off], note);
        }
        if (off == 1) rc = rc ? rc : arm<256>(src, dm, dout, cus, 4, reps, want_count[off], want_sum[off], note);
        if (off == 0) rc = rc ? rc : arm<512>(src, dm, dout, cus, 4, reps, want_count[off], want_sum[off], note);
        if (off == 0) rc = rc ? rc : arm<512>(src, dm, dout, cus, 8, reps, want_count[off], want_sum[off], note);
        if (rc) return rc;
    }
    return 0;
}
