// Host build of tinysql_amd/csrc/tsq_rowenc_dp.h for tests/test_rowenc_cpu.py: the per-row arithmetic of the write-path kernels, line
// by line.  Reads
//   v <type> <bits>                                  -> <width> <the value bytes as hex>          (F32: bits = the float32's 32 bits)
//   b <hex>                                          -> <ok 0|1> <value>                          (a bit column's cell)
//   r <id_large 0|1> <n_notnull> <n_null> <vbytes>   -> <large 0|1> <row length> <the six header bytes as hex>
//   u <hex>                                          -> <rune count>
//   p <prefix_len> <utf8 0|1> <hex>                  -> <bytes kept> <bad 0|1>
// ("-" = the empty cell)
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_rowenc_dp.h"

static std::vector<uint8_t> unhex(const char* s) {
    std::vector<uint8_t> out;
    const std::string hex = s[0] == '-' ? "" : s;
    for (size_t i = 0; i + 1 < hex.size(); i += 2) out.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
    return out;
}

int main() {
    static char buf[1 << 16];
    char op;
    while (scanf(" %c", &op) == 1) {
        if (op == 'v') {
            int type;
            unsigned long long bits;
            if (scanf("%d %llu", &type, &bits) != 2) return 2;
            uint64_t b = bits;
            if (type == TSQ_F32) b = tsq_f64_bits((double)tsq_bits_f32((uint32_t)bits));
            uint64_t le;
            const uint32_t w = tsq_re_value(type, b, &le);
            printf("%u ", w);
            for (uint32_t i = 0; i < w; i++) printf("%02x", (unsigned)((le >> (8 * i)) & 0xff));
            printf("\n");
        } else if (op == 'b') {
            if (scanf("%65535s", buf) != 1) return 2;
            // an exact-size heap copy: the sanitizer sees any read past the cell
            const std::vector<uint8_t> cell = unhex(buf);
            uint8_t* p = (uint8_t*)malloc(cell.size() ? cell.size() : 1);
            for (size_t i = 0; i < cell.size(); i++) p[i] = cell[i];
            uint64_t v;
            const bool ok = tsq_re_bit_value(p, cell.size(), &v);
            printf("%d %llu\n", ok ? 1 : 0, (unsigned long long)v);
            free(p);
        } else if (op == 'r') {
            int id_large;
            unsigned nn, nnull;
            unsigned long long vb;
            if (scanf("%d %u %u %llu", &id_large, &nn, &nnull, &vb) != 4) return 2;
            const bool large = tsq_re_large(id_large != 0, vb);
            const uint64_t hdr = tsq_re_header(large, nn, nnull);
            printf("%d %llu ", large ? 1 : 0, (unsigned long long)tsq_re_row_len(large, nn, nnull, vb));
            for (int i = 0; i < 6; i++) printf("%02x", (unsigned)((hdr >> (8 * i)) & 0xff));
            printf("\n");
        } else if (op == 'u' || op == 'p') {
            long long k = 0;
            int utf8 = 0;
            if (op == 'p' && scanf("%lld %d", &k, &utf8) != 2) return 2;
            if (scanf("%65535s", buf) != 1) return 2;
            const std::vector<uint8_t> cell = unhex(buf);
            uint8_t* p = (uint8_t*)malloc(cell.size() ? cell.size() : 1);
            for (size_t i = 0; i < cell.size(); i++) p[i] = cell[i];
            if (op == 'u') {
                printf("%llu\n", (unsigned long long)tsq_re_rune_count(p, cell.size()));
            } else {
                bool bad;
                const uint64_t kept = tsq_re_index_cell_len(p, cell.size(), k, utf8 != 0, &bad);
                printf("%llu %d\n", (unsigned long long)kept, bad ? 1 : 0);
            }
            free(p);
        } else {
            return 2;
        }
    }
    return 0;
}
