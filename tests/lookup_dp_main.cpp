// Host build of tinysql_amd/csrc/tsq_lookup_dp.h for tests/test_lookup_cpu.py: the plan of the sampled search index, its levels
// (built with the kernel's own sample arithmetic) and the descent, over exactly sized arrays so that the sanitizers see any index
// that leaves its level.  Reads from stdin:
//   T <n> <handles as signed decimals...>     the table
//   Q <m> <values...>                          what is searched
//   S <shift> <top_max>                        builds the index and prints one line: "<levels> <lower bound of every value...>"
//   F <shift> <top_max>                        the same through tsq_lk_find: "<levels> <row or -1 ...>"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <vector>

#include "../tinysql_amd/csrc/tsq_lookup_dp.h"

int main() {
    std::unique_ptr<int64_t[]> table(new int64_t[0]);
    long long n = 0;
    std::vector<int64_t> q;
    char op[8];
    while (scanf("%7s", op) == 1) {
        if (op[0] == 'T' || op[0] == 'Q') {
            long long m;
            if (scanf("%lld", &m) != 1 || m < 0) return 2;
            std::vector<int64_t> v((size_t)m);
            for (long long i = 0; i < m; i++) {
                long long x;
                if (scanf("%lld", &x) != 1) return 2;
                v[(size_t)i] = (int64_t)x;
            }
            if (op[0] == 'Q') {
                q.swap(v);
            } else {
                n = m;
                table.reset(new int64_t[(size_t)m]);  // exactly n entries
                if (m) memcpy(table.get(), v.data(), (size_t)m * 8);
            }
        } else if (op[0] == 'S' || op[0] == 'F') {
            int shift;
            long long top_max;
            if (scanf("%d %lld", &shift, &top_max) != 2) return 2;
            tsq_lk_index ix;
            memset(&ix, 0, sizeof ix);
            const int levels = tsq_lk_plan(&ix, n, shift, top_max);
            std::vector<std::unique_ptr<int64_t[]>> lv((size_t)levels + 1);
            ix.lv[0] = table.get();
            for (int k = 1; k <= levels; k++) {
                lv[(size_t)k].reset(new int64_t[(size_t)ix.n[k]]);
                for (int64_t j = 0; j < ix.n[k]; j++) {
                    const int64_t s = tsq_lk_sample_src(j, ix.shift);
                    if (s >= ix.n[k - 1]) return 3;  // the plan promised a source entry for every sample
                    lv[(size_t)k][(size_t)j] = ix.lv[k - 1][s];
                }
                ix.lv[k] = lv[(size_t)k].get();
            }
            printf("%d", levels);
            for (int64_t x : q) printf(" %lld", (long long)(op[0] == 'S' ? tsq_lk_search(ix, ix.lv[ix.levels], x) : tsq_lk_find(ix, ix.lv[ix.levels], x)));
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
