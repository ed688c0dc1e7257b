// Host build of tinysql_amd/csrc/tsq_unionscan_dp.h for tests/test_unionscan_cpu.py: the handle set (build + probe), the streaming
// bound, the diagonal search and the per-lane merge of the union-scan kernels, run over exactly sized arrays so that the sanitizers
// see any index that leaves its run.  Reads cases:
//   case <n_cols> <types...> | <handle_col> <desc> <n_keys> <key cols...> | <lane> <lanes per tile> <finish 0|1>
//   set <n> <handles as signed decimals...>
//   S <nrows>   then one line per row     A <nrows>   then one line per row
//       a cell: N = NULL | the 64 (F32: 32) bits as an unsigned decimal | x<hex> = a string's bytes ("x" alone: empty)
//   go
// and prints per case:  "kept <physical rows...>"  and  "take <m> <entries...>"  (s<row> = snapshot, a<row> = added).
// finish 0: the snapshot rows merge with the m added rows that precede the last kept row (the streaming rule); 1: with all.
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_unionscan_dp.h"

struct Side {
    int64_t n = 0;
    std::vector<std::unique_ptr<uint8_t[]>> data, nulls;
    std::vector<std::unique_ptr<int64_t[]>> offs;
    tsq_colset cs;
};

static bool read_side(Side& s, int n_cols, const int* types) {
    long long n;
    if (scanf("%lld", &n) != 1) return false;
    s.n = n;
    std::vector<std::vector<std::string>> cells(n_cols, std::vector<std::string>(n));
    static char buf[1 << 12];
    for (long long r = 0; r < n; r++)
        for (int c = 0; c < n_cols; c++) {
            if (scanf("%4095s", buf) != 1) return false;
            cells[c][r] = buf;
        }
    memset(&s.cs, 0, sizeof s.cs);
    s.cs.n = n_cols;
    s.data.resize(n_cols);
    s.nulls.resize(n_cols);
    s.offs.resize(n_cols);
    for (int c = 0; c < n_cols; c++) {
        s.cs.type[c] = types[c];
        bool any_null = false;
        for (auto& v : cells[c]) any_null = any_null || v == "N";
        if (any_null) {  // exactly (n + 7) / 8 bytes
            s.nulls[c].reset(new uint8_t[(n + 7) / 8]());
            for (long long r = 0; r < n; r++)
                if (cells[c][r] != "N") s.nulls[c][r >> 3] |= (uint8_t)(1u << (r & 7));
            s.cs.nulls[c] = s.nulls[c].get();
        }
        if (types[c] == TSQ_BYTES) {
            s.offs[c].reset(new int64_t[n + 1]());
            std::vector<uint8_t> bytes;
            for (long long r = 0; r < n; r++) {
                const std::string& v = cells[c][r];
                if (v != "N")
                    for (size_t i = 1; i + 1 < v.size(); i += 2) bytes.push_back((uint8_t)strtoul(v.substr(i, 2).c_str(), nullptr, 16));
                s.offs[c][r + 1] = (int64_t)bytes.size();
            }
            s.data[c].reset(new uint8_t[bytes.size() ? bytes.size() : 1]);
            if (!bytes.empty()) memcpy(s.data[c].get(), bytes.data(), bytes.size());
            s.cs.offs[c] = s.offs[c].get();
        } else {
            const int es = types[c] == TSQ_F32 ? 4 : 8;
            s.data[c].reset(new uint8_t[n ? n * es : 1]());
            for (long long r = 0; r < n; r++) {
                if (cells[c][r] == "N") continue;
                const uint64_t bits = strtoull(cells[c][r].c_str(), nullptr, 10);
                memcpy(s.data[c].get() + r * es, &bits, es);
            }
        }
        s.cs.data[c] = s.data[c].get();
    }
    return true;
}

int main() {
    char word[16];
    int n_cols = 0, types[TSQ_MAX_COLS], lane = 8, lanes_per_tile = 256, finish = 1;
    tsq_us_order order;
    std::vector<int64_t> handles;
    Side S, A;
    while (scanf("%15s", word) == 1) {
        const std::string w = word;
        if (w == "case") {
            memset(&order, 0, sizeof order);
            if (scanf("%d", &n_cols) != 1 || n_cols < 1 || n_cols > TSQ_MAX_COLS) return 2;
            for (int c = 0; c < n_cols; c++)
                if (scanf("%d", &types[c]) != 1) return 2;
            if (scanf("%d %d %d", &order.handle_col, &order.desc, &order.n_keys) != 3 || order.n_keys > TSQ_MAX_KEYS) return 2;
            for (int k = 0; k < order.n_keys; k++)
                if (scanf("%d", &order.key_col[k]) != 1) return 2;
            if (scanf("%d %d %d", &lane, &lanes_per_tile, &finish) != 3 || lane < 1 || lanes_per_tile < 1) return 2;
            handles.clear();
        } else if (w == "set") {
            long long n;
            if (scanf("%lld", &n) != 1) return 2;
            handles.resize(n);
            for (auto& h : handles) {
                long long v;
                if (scanf("%lld", &v) != 1) return 2;
                h = v;
            }
        } else if (w == "S") {
            if (!read_side(S, n_cols, types)) return 2;
        } else if (w == "A") {
            if (!read_side(A, n_cols, types)) return 2;
        } else if (w == "go") {
            // the set, exactly sized
            const uint64_t slots = tsq_us_set_slots(handles.size());
            std::unique_ptr<uint64_t[]> keys(new uint64_t[slots ? slots : 1]());
            std::unique_ptr<uint32_t[]> occ(new uint32_t[slots ? slots / 32 : 1]());
            for (int64_t h : handles) tsq_us_set_insert(keys.get(), occ.get(), slots, (uint64_t)h);
            tsq_us_set set{keys.get(), occ.get(), slots};
            std::unique_ptr<uint32_t[]> kept(new uint32_t[S.n ? S.n : 1]);
            int64_t nk = 0;
            for (int64_t r = 0; r < S.n; r++)
                if (!tsq_us_set_has(set, ((const uint64_t*)S.cs.data[order.handle_col])[r])) kept[nk++] = (uint32_t)r;
            printf("kept");
            for (int64_t i = 0; i < nk; i++) printf(" %u", kept[i]);
            printf("\n");
            tsq_us_view rs{kept.get(), 0, nk}, ra{nullptr, 0, A.n};
            int64_t m = A.n;
            if (!finish) m = nk ? tsq_us_bound(order, A.cs, ra, S.cs, tsq_us_phys(rs, nk - 1)) : 0;
            ra.n = m;
            const int64_t total = nk + m, tile = (int64_t)lane * lanes_per_tile;
            std::unique_ptr<uint32_t[]> take(new uint32_t[total ? total : 1]);
            for (int64_t i = 0; i < total; i++) take[i] = 0xffffffffu;
            for (int64_t d0 = 0; d0 < total; d0 += tile) {  // step 1: the splits of the tile's boundaries; step 2: its lanes
                const int64_t d1 = d0 + tile < total ? d0 + tile : total;
                tsq_us_view s, v;
                tsq_us_tile_views(rs, ra, d0, d1, tsq_us_diag(order, S.cs, rs, A.cs, ra, d0), tsq_us_diag(order, S.cs, rs, A.cs, ra, d1), &s, &v);
                for (int64_t d = 0; d < s.n + v.n; d += lane) tsq_us_lane_merge(order, S.cs, s, A.cs, v, d, tsq_us_diag(order, S.cs, s, A.cs, v, d), lane, take.get() + d0);
            }
            printf("take %lld", (long long)m);
            for (int64_t i = 0; i < total; i++) {
                if (take[i] == 0xffffffffu) printf(" ?");
                else printf(" %c%u", (take[i] & TSQ_US_SIDE_ADDED) ? 'a' : 's', take[i] & 0x7fffffffu);
            }
            printf("\n");
        } else {
            return 3;
        }
    }
    return 0;
}
