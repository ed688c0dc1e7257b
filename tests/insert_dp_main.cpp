// insert_dp_main.cpp — the per-cell arithmetic of the INSERT .. SELECT kernels (tinysql_amd/csrc/tsq_insert_dp.h, the very code the
// kernels run) as a stand-alone host program for tests/test_cast_cpu.py: built with -fsanitize=address,undefined -ffp-contract=off.
// One answer line per input line:
//   col <src_col> <src_type> <tp> <flen> <decimal> <col_flags> <stmt_flags> <def_bits hex> [<str_ctx>]
//                                   -> "<status of tsq_ins_plan_col>"; sets the column the x lines go through
//   x <in_null 0|1> <bits hex>      -> "<status> <phase> <out_null> <bits hex> <overflow warnings> <bad-null warnings>"
//                                      (a string column: the integer is formatted first; the answer has the form of y's)
//   y <in_null 0|1> <bytes hex | ->  -> "<status> <phase> <out_null> <cell bytes hex | -> <bad-null> <data-too-long> <bad-utf8 warnings>"
//   z <in_null 0|1> <bytes hex | ->  -> a string cell into an INTEGER column: "<status> <phase> <out_null> <bits hex> <overflow> <bad-null> <truncated warnings>"
//   p <n>                           -> "<bits hex of math.Pow10(n)>"
//   a <base> <flags> <upper> <seed> <n> <v | N> ...
//                                   -> "<ovf> <new_base> <first bad row | -1> id ..." : every prefix operator composed under a random bracketing
#include <cinttypes>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <sstream>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_insert_dp.h"

static uint64_t rng_state;
static uint64_t rnd() { return rng_state = tsq_splitmix64(rng_state); }

// the operators of rows [lo, hi) composed along a random tree
static tsq_aid_op compose_range(const std::vector<tsq_aid_op>& ops, size_t lo, size_t hi) {
    if (hi == lo) return tsq_aid_identity();
    if (hi - lo == 1) return ops[lo];
    const size_t mid = lo + 1 + (size_t)(rnd() % (hi - lo - 1));
    return tsq_aid_compose(compose_range(ops, lo, mid), compose_range(ops, mid, hi));
}

int main() {
    tsq_ins_col col;
    memset(&col, 0, sizeof col);
    uint32_t stmt_flags = 0, str_ctx = 0;
    std::string line;
    char buf[1 << 16];
    while (fgets(buf, sizeof buf, stdin)) {
        std::istringstream in(buf);
        std::string cmd;
        in >> cmd;
        if (cmd == "col") {
            tsq_cast_col s;
            memset(&s, 0, sizeof s);
            std::string def;
            in >> s.src_col >> s.src_type >> s.tp >> s.flen >> s.decimal >> s.flags >> stmt_flags >> def;
            s.def_bits = strtoull(def.c_str(), nullptr, 16);
            str_ctx = 0;
            in >> str_ctx;
            const char* why;
            printf("%d\n", (int)tsq_ins_plan_col(s, &col, &why));
        } else if (cmd == "y" || (cmd == "x" && col.kind == TSQ_INS_STR)) {
            int in_null;
            std::string hex;
            in >> in_null >> hex;
            std::vector<uint8_t> src;
            if (cmd == "y") {
                if (hex != "-")
                    for (size_t i = 0; i + 1 < hex.size(); i += 2) src.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
            } else {
                uint64_t w0, w1, w2;
                const uint32_t n = tsq_ins_format_int(col.src_type, strtoull(hex.c_str(), nullptr, 16), &w0, &w1, &w2);
                for (uint32_t i = 0; i < n; i++) src.push_back(tsq_ins_fmt_byte(w0, w1, w2, i));
                // the shortcut for formatted integers must agree with the general walk over the same bytes
                uint64_t k1, p1, k2, p2;
                uint32_t e1 = 0, e2 = 0;
                tsq_ins_str_shape_ascii(col, n, &k1, &p1, &e1);
                tsq_ins_str_shape(col, stmt_flags | TSQ_CAST_IGNORE_TRUNCATE, src.data(), n, &k2, &p2, &e2);
                if (k1 != k2 || p1 != p2 || e1 != e2) { printf("ascii shape differs\n"); continue; }
            }
            uint64_t keep = 0, pad = 0;
            bool from_default = false, out_null = false;
            int32_t status = 0, phase = 0;
            uint32_t w[4] = {0, 0, 0, 0};
            src.push_back(0);  // (never read: keeps data() non-null for an empty string)
            tsq_ins_str_cell(col, stmt_flags, src.data(), src.size() - 1, in_null != 0, &keep, &pad, &from_default, &out_null, &status, &phase, w);
            std::string cell;
            char b2[3];
            for (uint64_t i = 0; i < keep && !from_default; i++) { snprintf(b2, 3, "%02x", src[i]); cell += b2; }
            for (uint64_t i = 0; i < pad; i++) cell += "00";
            printf("%d %d %d %s %u %u %u\n", status, phase, out_null ? 1 : 0, cell.empty() ? "-" : cell.c_str(), w[1], w[2], w[3]);
        } else if (cmd == "x") {
            int in_null;
            std::string hex;
            in >> in_null >> hex;
            bool out_null = false;
            int32_t status = 0, phase = 0;
            uint32_t w0 = 0, w1 = 0;
            const uint64_t v = tsq_ins_cell(col, stmt_flags, strtoull(hex.c_str(), nullptr, 16), in_null != 0, &out_null, &status, &phase, &w0, &w1);
            printf("%d %d %d %" PRIx64 " %u %u\n", status, phase, out_null ? 1 : 0, v, w0, w1);
        } else if (cmd == "z") {
            int in_null;
            std::string hex;
            in >> in_null >> hex;
            std::vector<uint8_t> src;
            if (hex != "-")
                for (size_t i = 0; i + 1 < hex.size(); i += 2) src.push_back((uint8_t)strtoul(hex.substr(i, 2).c_str(), nullptr, 16));
            const uint32_t n = (uint32_t)src.size();
            uint8_t* exact = (uint8_t*)malloc(n ? n : 1);  // exactly n bytes: a read past the cell is the sanitizer's to report
            if (n) memcpy(exact, src.data(), n);
            bool out_null = false;
            int32_t status = 0, phase = 0;
            uint32_t w[3] = {0, 0, 0};
            const uint64_t v = tsq_ins_cell_str_int(col, stmt_flags, str_ctx, exact, n, in_null != 0, &out_null, &status, &phase, w);
            free(exact);
            printf("%d %d %d %" PRIx64 " %u %u %u\n", status, phase, out_null ? 1 : 0, v, w[0], w[1], w[2]);
        } else if (cmd == "p") {
            int n;
            in >> n;
            printf("%" PRIx64 "\n", tsq_f64_bits(tsq_ins_pow10(n)));
        } else if (cmd == "a") {
            int64_t base, upper;
            uint32_t flags;
            size_t n;
            in >> base >> flags >> upper >> rng_state >> n;
            std::vector<int64_t> v(n);
            std::vector<int> kind(n);
            std::vector<tsq_aid_op> ops(n);
            for (size_t i = 0; i < n; i++) {
                std::string t;
                in >> t;
                const bool isnull = t == "N";
                v[i] = isnull ? 0 : (int64_t)strtoll(t.c_str(), nullptr, 10);
                kind[i] = tsq_aid_row_kind(v[i], isnull, flags);
                ops[i] = tsq_aid_row_op(kind[i], v[i]);
            }
            int32_t ovf = 0;
            int64_t bad = -1;
            std::string ids;
            for (size_t i = 0; i < n; i++) {
                int32_t o = 0;
                const int64_t s = tsq_aid_apply(compose_range(ops, 0, i + 1), base, &o);
                ovf |= o;
                const int64_t id = kind[i] == TSQ_AID_ALLOC ? s : v[i];
                if (kind[i] == TSQ_AID_ALLOC && s > upper && bad < 0) bad = (int64_t)i;
                ids += " " + std::to_string(id);
            }
            int32_t o = 0;
            const int64_t nb = tsq_aid_apply(compose_range(ops, 0, n), base, &o);
            printf("%d %" PRId64 " %" PRId64 "%s\n", ovf | o, nb, bad, ids.c_str());
        } else {
            printf("?\n");
        }
    }
    return 0;
}
