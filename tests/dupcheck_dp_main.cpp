// Host build of tinysql_amd/csrc/tsq_dupcheck_dp.h for tests/test_dupcheck_cpu.py: the key compare, the lower bound over a store's
// keys and the cell equality of tsq_rows_equal, over exactly sized heap arrays so that the sanitizers see any byte read past a key or
// a cell.  Reads from stdin (keys and cells as hex, "-" for the empty string):
//   K <n> <key...>        the store's keys, in order
//   P <m> <key...>        probes; prints one line "<find> <lower>" per probe
//   C <a> <b>             prints "<sign of tsq_dc_key_cmp> <tsq_dc_bytes_equal>", each key in an allocation of its own
//   D <bits a> <bits b>   two doubles by their bits (hex); prints tsq_dc_cell_equal as TSQ_F64
//   S <na> <a> <nb> <b>   two string cells, na / nb = 1 when the cell is NULL; prints tsq_dc_cell_equal as TSQ_BYTES
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_dupcheck_dp.h"

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> v;
    if (s[0] == '-') return v;
    for (size_t i = 0; s[i] && s[i + 1]; i += 2) {
        unsigned x;
        sscanf(s + i, "%2x", &x);
        v.push_back((uint8_t)x);
    }
    return v;
}
static std::unique_ptr<uint8_t[]> exact(const std::vector<uint8_t>& v) {
    std::unique_ptr<uint8_t[]> p(new uint8_t[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size());
    return p;
}

int main() {
    std::unique_ptr<uint8_t[]> keys(new uint8_t[0]);
    std::unique_ptr<int64_t[]> offs(new int64_t[1]);
    offs[0] = 0;
    long long n = 0;
    char op[8];
    static char buf[1 << 16], buf2[1 << 16];
    while (scanf("%7s", op) == 1) {
        if (op[0] == 'K') {
            if (scanf("%lld", &n) != 1 || n < 0) return 2;
            std::vector<uint8_t> all;
            offs.reset(new int64_t[(size_t)n + 1]);
            offs[0] = 0;
            for (long long i = 0; i < n; i++) {
                if (scanf("%65535s", buf) != 1) return 2;
                const std::vector<uint8_t> k = unhex(buf);
                all.insert(all.end(), k.begin(), k.end());
                offs[(size_t)i + 1] = (int64_t)all.size();
            }
            keys = exact(all);
        } else if (op[0] == 'P') {
            long long m;
            if (scanf("%lld", &m) != 1 || m < 0) return 2;
            for (long long i = 0; i < m; i++) {
                if (scanf("%65535s", buf) != 1) return 2;
                const std::vector<uint8_t> k = unhex(buf);
                const std::unique_ptr<uint8_t[]> p = exact(k);
                printf("%lld %lld\n", (long long)tsq_dc_key_find(keys.get(), offs.get(), n, p.get(), (int64_t)k.size()),
                       (long long)tsq_dc_key_lower(keys.get(), offs.get(), n, p.get(), (int64_t)k.size()));
            }
        } else if (op[0] == 'C') {
            if (scanf("%65535s %65535s", buf, buf2) != 2) return 2;
            const std::vector<uint8_t> a = unhex(buf), b = unhex(buf2);
            const std::unique_ptr<uint8_t[]> pa = exact(a), pb = exact(b);
            const int c = tsq_dc_key_cmp(pa.get(), (int64_t)a.size(), pb.get(), (int64_t)b.size());
            printf("%d %d\n", c < 0 ? -1 : (c > 0 ? 1 : 0), tsq_dc_bytes_equal(pa.get(), (int64_t)a.size(), pb.get(), (int64_t)b.size()) ? 1 : 0);
        } else if (op[0] == 'D') {
            unsigned long long x, y;
            if (scanf("%llx %llx", &x, &y) != 2) return 2;
            std::unique_ptr<uint64_t[]> pa(new uint64_t[1]), pb(new uint64_t[1]);
            pa[0] = x;
            pb[0] = y;
            const tsq_dc_col a = {pa.get(), nullptr, nullptr, 1}, b = {pb.get(), nullptr, nullptr, 1};
            printf("%d\n", tsq_dc_cell_equal(TSQ_F64, a, 0, b, 0) ? 1 : 0);
        } else if (op[0] == 'S') {
            int na, nb;
            if (scanf("%d %65535s %d %65535s", &na, buf, &nb, buf2) != 4) return 2;
            const std::vector<uint8_t> va = unhex(buf), vb = unhex(buf2);
            const std::unique_ptr<uint8_t[]> pa = exact(va), pb = exact(vb);
            std::unique_ptr<int64_t[]> oa(new int64_t[2]), ob(new int64_t[2]);
            oa[0] = ob[0] = 0;
            oa[1] = (int64_t)va.size();
            ob[1] = (int64_t)vb.size();
            std::unique_ptr<uint8_t[]> ba(new uint8_t[1]), bb(new uint8_t[1]);
            ba[0] = na ? 0 : 1;
            bb[0] = nb ? 0 : 1;
            const tsq_dc_col a = {pa.get(), ba.get(), oa.get(), 1}, b = {pb.get(), bb.get(), ob.get(), 1};
            printf("%d\n", tsq_dc_cell_equal(TSQ_BYTES, a, 0, b, 0) ? 1 : 0);
        } else {
            return 2;
        }
    }
    return 0;
}
