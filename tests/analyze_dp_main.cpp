// Host build of tinysql_amd/csrc/tsq_analyze_dp.h for tests/test_analyze_cpu.py: reads lines
//   <type> <col_flags> <null: 0|1> <value: integer bits, or the cell as hex, "-" = empty>
// and prints per line:  len(e)  h1  h2  fm_hash_unwrapped  fm_hash_wrapped   (hex) — the kernel's per-cell arithmetic, line by line.
#include <cstdio>
#include <cstdlib>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_analyze_dp.h"

int main() {
    char buf[1 << 16];
    int type;
    unsigned flags;
    int null;
    while (scanf("%d %u %d %65535s", &type, &flags, &null, buf) == 4) {
        const bool comparable = flags & TSQ_ENC_COMPARABLE, raw = flags & TSQ_AN_RAW;
        tsq_mm3 m, w;
        uint64_t elen;
        std::vector<uint8_t> cell;
        if (type == TSQ_BYTES) {
            const std::string hex = buf[0] == '-' ? "" : buf;
            for (size_t i = 0; i + 1 < hex.size(); i += 2) cell.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
            const tsq_an_bytes e = tsq_an_cell(cell.data(), cell.size(), raw, comparable);
            m = tsq_an_hash(e);
            w = tsq_an_hash(tsq_an_wrap(e));
            elen = tsq_an_len(e);
        } else {
            uint64_t bits = strtoull(buf, nullptr, 10);
            if (type == TSQ_F32) bits = tsq_f64_bits((double)tsq_bits_f32((uint32_t)bits));
            uint64_t lo;
            uint32_t hi;
            const uint32_t len = tsq_enc_bytes(type, comparable, bits, true, &lo, &hi);
            m = tsq_mm3_short(lo, hi, len);
            w = tsq_an_hash_fixed_wrapped(lo, hi, len);
            elen = len;
        }
        printf("%llu %llx %llx %llx %llx\n", (unsigned long long)elen, (unsigned long long)m.h1, (unsigned long long)m.h2, (unsigned long long)m.h1,
               (unsigned long long)w.h1);
    }
    return 0;
}
