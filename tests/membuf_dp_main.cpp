// Host build of tinysql_amd/csrc/tsq_membuf_dp.h for tests/test_membuf_cpu.py: the checks of every pushed row, the survey (lengths,
// shared prefix, "already ascending"), the order — in the LANE form, a comparison sort under tsq_mb_entry_cmp, and in the WAVE form,
// the stable radix passes over the tuple's images that k_mb_image / k_mb_scatter of tsq_membuf.hip run, ranks taken 64 lanes at a
// time as the ballots do; the program fails when the two orders differ — the winner rule and the search of a Get, over exactly sized
// heap arrays so that the sanitizers see any read past a key or an array.
// Reads from stdin (keys as hex, "-" for the empty string):
//   B <entry size limit> <pushes>        then per push:  P <kind> <n>  and n lines <key> <value length>
//                                        a refused push prints "E <push> <error bits> <first row>" and adds nothing
//                                        then prints "R <entries> <prefix> <depths> <ascending> <passes>" and per entry
//                                        <op> <key> <value length> <sequence number>
//   G <n>                                then n lines <key>; prints "G" and n lines <entry index or -1>
#include <algorithm>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_membuf_dp.h"

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
static std::string hex(const uint8_t* p, int64_t n) {
    if (n == 0) return "-";
    static const char* d = "0123456789abcdef";
    std::string s;
    for (int64_t i = 0; i < n; i++) {
        s.push_back(d[p[i] >> 4]);
        s.push_back(d[p[i] & 15]);
    }
    return s;
}
template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

static char buf[1 << 16];

// the entries by sequence number: every key in its own exactly sized block, laid out through one byte array as the device has them
struct Entries {
    std::vector<uint8_t> bytes;
    std::vector<int64_t> kbeg, klen, vlen;
    std::vector<uint8_t> kind;
};

int main() {
    Entries en;
    std::unique_ptr<uint8_t[]> okeys;
    std::unique_ptr<int64_t[]> okoff;
    int64_t m = 0;
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'B') {
            long long limit, pushes;
            if (scanf("%lld %lld", &limit, &pushes) != 2) return 2;
            en = Entries();
            for (long long pi = 0; pi < pushes; pi++) {
                int kind;
                long long n;
                if (scanf("%7s %d %lld", cmd, &kind, &n) != 3 || cmd[0] != 'P') return 2;
                std::vector<uint8_t> kb;
                std::vector<int64_t> koff(1, 0), voff(1, 0);
                for (long long i = 0; i < n; i++) {
                    long long vl;
                    if (scanf("%65535s %lld", buf, &vl) != 2) return 2;
                    const std::vector<uint8_t> k = unhex(buf);
                    kb.insert(kb.end(), k.begin(), k.end());
                    koff.push_back((int64_t)kb.size());
                    voff.push_back(voff.back() + vl);
                }
                auto xko = exact(koff), xvo = exact(voff);
                tsq_mb_push_view p;
                p.koff = xko.get(), p.fixed_len = 0, p.key_bytes = (int64_t)kb.size(), p.voff = kind == TSQ_MEMBUF_SET ? xvo.get() : nullptr;
                p.value_bytes = kind == TSQ_MEMBUF_SET ? voff.back() : 0, p.n = n, p.kind = kind, p.entry_limit = limit;
                // keys of one length: the same rows once more through the fixed-length form, which must agree
                bool fixed = n > 0;
                for (long long i = 0; i < n && fixed; i++) fixed = koff[i + 1] - koff[i] == koff[1] - koff[0];
                tsq_mb_push_view pf = p;
                pf.koff = nullptr, pf.fixed_len = fixed ? koff[1] - koff[0] : 0;
                unsigned bits = 0;
                long long first = -1;
                std::vector<int64_t> b(n), l(n), vl(n);
                for (long long i = 0; i < n; i++) {
                    int64_t vb;
                    const uint32_t e = tsq_mb_push_check(p, i, &b[i], &l[i], &vb, &vl[i]);
                    if (fixed) {
                        int64_t b2, l2, vb2, vl2;
                        if (tsq_mb_push_check(pf, i, &b2, &l2, &vb2, &vl2) != e || b2 != b[i] || l2 != l[i] || vl2 != vl[i]) {
                            printf("the fixed-length form differs at row %lld\n", i);
                            return 1;
                        }
                    }
                    bits |= e;
                    if (e && first < 0) first = i;
                }
                if (bits) {
                    printf("E %lld %u %lld\n", pi, bits, first);
                    continue;
                }
                const int64_t base = (int64_t)en.bytes.size();
                en.bytes.insert(en.bytes.end(), kb.begin(), kb.end());
                for (long long i = 0; i < n; i++) {
                    en.kbeg.push_back(base + b[i]);
                    en.klen.push_back(l[i]);
                    en.vlen.push_back(vl[i]);
                    en.kind.push_back((uint8_t)kind);
                }
            }
            // ---- finish
            const int64_t n = (int64_t)en.klen.size();
            auto keys = exact(en.bytes);
            auto kbeg = exact(en.kbeg), klen = exact(en.klen);
            int64_t mn = INT64_MAX, mx = 0, prefix = INT64_MAX;
            bool ascending = true;
            for (int64_t e = 0; e < n; e++) {
                mn = std::min(mn, klen[e]);
                mx = std::max(mx, klen[e]);
                prefix = std::min(prefix, tsq_mb_common_prefix(keys.get() + kbeg[0], klen[0], keys.get() + kbeg[e], klen[e], klen[0]));
                if (e > 0 && !tsq_mb_ascending_at(keys.get(), kbeg.get(), klen.get(), e)) ascending = false;
            }
            if (n == 0) prefix = 0;
            const int64_t depths = tsq_mb_depths(mx, prefix);
            // the lane form
            std::vector<uint32_t> lane_order(n);
            for (int64_t i = 0; i < n; i++) lane_order[i] = (uint32_t)i;
            std::sort(lane_order.begin(), lane_order.end(), [&](uint32_t x, uint32_t y) {
                return tsq_mb_entry_cmp(keys.get() + kbeg[x], klen[x], en.kind[x], x, keys.get() + kbeg[y], klen[y], en.kind[y], y, prefix, depths) < 0;
            });
            // the wave form
            std::vector<uint32_t> idx(n), idx2(n);
            std::vector<uint64_t> img(n), img2(n);
            for (int64_t i = 0; i < n; i++) idx[i] = (uint32_t)i;
            long long passes = 0;
            for (int64_t step = 0, d = -1; step <= depths && n > 1 && !ascending; step++, d = depths - step) {
                uint64_t vor = 0, vand = ~0ull;
                for (int64_t i = 0; i < n; i++) {
                    const uint32_t e = idx[i];
                    img[i] = d < 0 ? tsq_mb_tail_image(klen[e], prefix, en.kind[e]) : tsq_mb_image(keys.get() + kbeg[e], klen[e], prefix, d);
                    vor |= img[i];
                    vand &= img[i];
                }
                for (int digit = 0; digit < 8; digit++) {
                    if (!(((vor ^ vand) >> (8 * digit)) & 255)) continue;
                    std::vector<int64_t> count(257, 0), run(256, 0);
                    for (int64_t i = 0; i < n; i++) count[((img[i] >> (8 * digit)) & 255) + 1]++;
                    for (int q = 0; q < 256; q++) count[q + 1] += count[q];
                    for (int64_t g = 0; g < n; g += 64) {  // one wave step: the rank of a lane = the running count + the equal digits in front of it
                        const int64_t ge = std::min<int64_t>(g + 64, n);
                        int64_t in_step[256] = {0};
                        for (int64_t i = g; i < ge; i++) {
                            const int dg = (int)((img[i] >> (8 * digit)) & 255);
                            const int64_t before = in_step[dg]++;
                            const int64_t dst = count[dg] + run[dg] + before;
                            img2[dst] = img[i];
                            idx2[dst] = idx[i];
                        }
                        for (int64_t i = g; i < ge; i++) run[(img[i] >> (8 * digit)) & 255]++;
                    }
                    img.swap(img2);
                    idx.swap(idx2);
                    passes++;
                }
            }
            if (idx != lane_order) {
                printf("the order of the radix passes differs from the comparison sort's\n");
                return 1;
            }
            for (int64_t i = 1; i < n; i++) {  // ... and both from bytes.Compare
                const uint32_t x = idx[i - 1], y = idx[i];
                if (tsq_dc_key_cmp(keys.get() + kbeg[x], klen[x], keys.get() + kbeg[y], klen[y]) > 0) {
                    printf("the order differs from bytes.Compare at %lld\n", (long long)i);
                    return 1;
                }
            }
            auto order = exact(idx);
            tsq_mb_sorted s;
            s.keys = keys.get(), s.kbeg = kbeg.get(), s.klen = klen.get(), s.order = order.get(), s.n = n, s.prefix = prefix;
            std::vector<uint32_t> win;
            for (int64_t i = 0; i < n; i++)
                if (tsq_mb_is_winner(s, i)) win.push_back(order[i]);
            m = (int64_t)win.size();
            printf("R %lld %lld %lld %d %lld\n", (long long)m, (long long)prefix, (long long)depths, ascending ? 1 : 0, passes);
            std::vector<uint8_t> ok;
            std::vector<int64_t> oo(1, 0);
            for (uint32_t e : win) {
                printf("%d %s %lld %u\n", (int)en.kind[e], hex(keys.get() + kbeg[e], klen[e]).c_str(), (long long)(en.kind[e] == TSQ_MEMBUF_SET ? en.vlen[e] : 0), e);
                ok.insert(ok.end(), keys.get() + kbeg[e], keys.get() + kbeg[e] + klen[e]);
                oo.push_back((int64_t)ok.size());
            }
            okeys = exact(ok);
            okoff = exact(oo);
        } else if (cmd[0] == 'G') {
            long long n;
            if (scanf("%lld", &n) != 1) return 2;
            printf("G\n");
            for (long long i = 0; i < n; i++) {
                if (scanf("%65535s", buf) != 1) return 2;
                const std::vector<uint8_t> k = unhex(buf);
                auto xk = exact(k);
                printf("%lld\n", (long long)tsq_mb_find(okeys.get(), okoff.get(), m, xk.get(), (int64_t)k.size()));
            }
        } else {
            return 2;
        }
    }
    return 0;
}
