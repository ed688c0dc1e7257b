// Host build of tinysql_amd/csrc/tsq_mvcc_dp.h for tests/test_mvcc_cpu.py: the create checks, the key universe, the bound search,
// the lock check and the chain walk — by one lane and in the wave form, emulated lane by lane — run in the order tsq_mvcc.hip runs
// them, over exactly sized heap arrays so that the sanitizers see any read past a key, a chain or an array.
// Reads from stdin (keys as hex, "-" for the empty string):
//   S <n> <n_locks>                       then n lines  <key> <commitTS> <type> <value length>
//                                         and n_locks lines <key> <startTS> <op> <primary>
//                                         prints "E <error bits>" or "U <keys of the universe>"
//   Q <ts> <desc> <limit> <chain> <R>     then R lines <start> <end> <flags>; limit < 0: none; chain: the wave threshold (<= 0: never)
//                                         prints "R <0 | 17> <pairs> <entry of the locked key's lock or -1>", the chosen entries, the range counts
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_mvcc_dp.h"

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
template <class T>
static std::unique_ptr<T[]> exact(const std::vector<T>& v) {
    std::unique_ptr<T[]> p(new T[v.size()]);
    if (!v.empty()) memcpy(p.get(), v.data(), v.size() * sizeof(T));
    return p;
}

struct Store {
    std::unique_ptr<uint8_t[]> keys, types, lops, lprim;
    std::unique_ptr<int64_t[]> koff, voff, lkoff, lpoff, ubeg;
    std::unique_ptr<uint64_t[]> cts, lstart;
    std::unique_ptr<int32_t[]> ulen, useg, ucnt, ulock;
    int64_t n = 0, nl = 0, U = 0;
    bool ok = false;
};

static char buf[1 << 16], buf2[1 << 16];

static bool read_store(Store& s) {
    long long n, nl;
    if (scanf("%lld %lld", &n, &nl) != 2 || n < 0 || nl < 0) return false;
    std::vector<uint8_t> kb, lkb, types, lops, prim;
    std::vector<int64_t> koff(1, 0), voff(1, 0), lkoff(1, 0), lpoff(1, 0);
    std::vector<uint64_t> cts, lstart;
    for (long long i = 0; i < n; i++) {
        unsigned long long c;
        int t;
        long long vl;
        if (scanf("%65535s %llu %d %lld", buf, &c, &t, &vl) != 4) return false;
        const std::vector<uint8_t> k = unhex(buf);
        kb.insert(kb.end(), k.begin(), k.end());
        koff.push_back((int64_t)kb.size());
        cts.push_back(c);
        types.push_back((uint8_t)t);
        voff.push_back(voff.back() + vl);
    }
    for (long long j = 0; j < nl; j++) {
        unsigned long long st;
        int op;
        if (scanf("%65535s %llu %d %65535s", buf, &st, &op, buf2) != 4) return false;
        const std::vector<uint8_t> k = unhex(buf), p = unhex(buf2);
        lkb.insert(lkb.end(), k.begin(), k.end());
        lkoff.push_back((int64_t)lkb.size());
        lstart.push_back(st);
        lops.push_back((uint8_t)op);
        prim.insert(prim.end(), p.begin(), p.end());
        lpoff.push_back((int64_t)prim.size());
    }
    const int64_t key_bytes = (int64_t)kb.size(), lkey_bytes = (int64_t)lkb.size();
    kb.insert(kb.end(), lkb.begin(), lkb.end());  // the store's keys, then the locks' keys
    s.keys = exact(kb);
    s.types = exact(types);
    s.lops = exact(lops);
    s.lprim = exact(prim);
    s.koff = exact(koff);
    s.voff = exact(voff);
    s.lkoff = exact(lkoff);
    s.lpoff = exact(lpoff);
    s.cts = exact(cts);
    s.lstart = exact(lstart);
    s.n = n;
    s.nl = nl;
    s.ok = false;
    // K21a / K21b
    uint32_t err = 0;
    std::vector<uint8_t> head((size_t)n);
    for (int64_t i = 0; i < n; i++) {
        bool h = true;
        err |= tsq_mv_entry_check(s.keys.get(), s.koff.get(), key_bytes, s.cts.get(), s.types.get(), s.voff.get(), voff.back(), i, &h);
        head[(size_t)i] = h ? 1 : 0;
    }
    for (int64_t j = 0; j < nl; j++)
        err |= tsq_mv_lock_entry_check(s.keys.get() + key_bytes, s.lkoff.get(), lkey_bytes, s.lops.get(), s.lpoff.get(), (int64_t)prim.size(), j);
    if (err) {
        printf("E %u\n", err);
        return true;
    }
    // the scan of the head flags, K21c
    std::unique_ptr<int32_t[]> seg(new int32_t[(size_t)n + 1]);
    seg[0] = 0;
    int64_t K = 0;
    for (int64_t i = 0; i < n; i++) {
        if (head[(size_t)i]) seg[(size_t)K++] = (int32_t)i;
    }
    seg[(size_t)K] = (int32_t)n;
    // K21d and the two scans
    std::unique_ptr<int64_t[]> add(new int64_t[(size_t)n + 2]()), rank(new int64_t[(size_t)nl + 1]());
    std::unique_ptr<int32_t[]> llb(new int32_t[(size_t)nl]);
    std::unique_ptr<uint8_t[]> leq(new uint8_t[(size_t)nl]);
    const uint8_t* lkeys = s.keys.get() + key_bytes;
    int64_t orphans = 0;
    std::vector<int64_t> per((size_t)n + 2, 0);
    for (int64_t j = 0; j < nl; j++) {
        const int64_t b = s.lkoff[(size_t)j], len = s.lkoff[(size_t)j + 1] - b;
        const int64_t lb = tsq_mv_lower_heads(s.keys.get(), s.koff.get(), seg.get(), K, lkeys + b, len);
        bool eq = false;
        if (lb < K) {
            const int64_t e = seg[(size_t)lb], kb0 = s.koff[(size_t)e];
            eq = tsq_dc_bytes_equal(s.keys.get() + kb0, s.koff[(size_t)e + 1] - kb0, lkeys + b, len);
        }
        llb[(size_t)j] = (int32_t)lb;
        leq[(size_t)j] = eq ? 1 : 0;
        rank[(size_t)j] = orphans;
        if (!eq) {
            orphans++;
            per[(size_t)lb]++;
        }
    }
    for (int64_t k = 0, run = 0; k < n + 2; k++) {  // exclusive
        add[(size_t)k] = run;
        run += per[(size_t)k];
    }
    // K21e / K21f
    const int64_t U = K + orphans;
    s.ubeg.reset(new int64_t[(size_t)U]);
    s.ulen.reset(new int32_t[(size_t)U]);
    s.useg.reset(new int32_t[(size_t)U]);
    s.ucnt.reset(new int32_t[(size_t)U]);
    s.ulock.reset(new int32_t[(size_t)U]);
    for (int64_t k = 0; k < K; k++) {
        const int64_t u = k + add[(size_t)k + 1], e = seg[(size_t)k];
        s.ubeg[(size_t)u] = s.koff[(size_t)e];
        s.ulen[(size_t)u] = (int32_t)(s.koff[(size_t)e + 1] - s.koff[(size_t)e]);
        s.useg[(size_t)u] = (int32_t)e;
        s.ucnt[(size_t)u] = seg[(size_t)k + 1] - (int32_t)e;
        s.ulock[(size_t)u] = -1;
    }
    for (int64_t j = 0; j < nl; j++) {
        const int64_t lb = llb[(size_t)j];
        if (leq[(size_t)j]) {
            s.ulock[(size_t)(lb + add[(size_t)lb + 1])] = (int32_t)j;
        } else {
            const int64_t u = lb + rank[(size_t)j];
            s.ubeg[(size_t)u] = key_bytes + s.lkoff[(size_t)j];
            s.ulen[(size_t)u] = (int32_t)(s.lkoff[(size_t)j + 1] - s.lkoff[(size_t)j]);
            s.useg[(size_t)u] = 0;
            s.ucnt[(size_t)u] = 0;
            s.ulock[(size_t)u] = (int32_t)j;
        }
    }
    s.U = U;
    s.ok = true;
    printf("U %lld\n", (long long)U);
    return true;
}

static bool query(const Store& s) {
    unsigned long long ts;
    int desc;
    long long limit, chain, R;
    if (scanf("%llu %d %lld %lld %lld", &ts, &desc, &limit, &chain, &R) != 5 || R < 0 || !s.ok) return false;
    tsq_mv_store v;
    v.k.bytes = s.keys.get();
    v.k.beg = s.ubeg.get();
    v.k.len = s.ulen.get();
    v.k.n = s.U;
    v.seg = s.useg.get();
    v.cnt = s.ucnt.get();
    v.lock = s.ulock.get();
    v.cts = s.cts.get();
    v.types = s.types.get();
    v.l_start = s.lstart.get();
    v.l_op = s.lops.get();
    v.l_prim = s.lprim.get();
    v.l_poff = s.lpoff.get();
    // K21g + the scan
    std::unique_ptr<int64_t[]> base(new int64_t[(size_t)R + 1]);
    std::unique_ptr<int32_t[]> rlo(new int32_t[(size_t)R]);
    int64_t P = 0;
    for (long long r = 0; r < R; r++) {
        unsigned fl;
        if (scanf("%65535s %65535s %u", buf, buf2, &fl) != 3) return false;
        const std::vector<uint8_t> a = unhex(buf), b = unhex(buf2);
        const std::unique_ptr<uint8_t[]> pa = exact(a), pb = exact(b);
        int64_t lo = 0, cnt = 0;
        tsq_mv_bounds(v.k, pa.get(), (int64_t)a.size(), pb.get(), (int64_t)b.size(), fl, &lo, &cnt);
        rlo[(size_t)r] = (int32_t)lo;
        base[(size_t)r] = P;
        P += cnt;
    }
    base[(size_t)R] = P;
    const int64_t lim = limit < 0 ? INT64_MAX : limit;
    // K21h
    std::unique_ptr<int32_t[]> chosen(new int32_t[(size_t)P]);
    int64_t first = -1, walked = 0;
    for (int64_t p = 0; p < P; p++) {
        const int64_t r = tsq_mv_range_of(base.get(), R, p), rb = base[(size_t)r];
        const int64_t u = tsq_mv_key_at(rlo[(size_t)r], base[(size_t)r + 1] - rb, p - rb, desc);
        uint64_t t = ts;
        int64_t res = -1;
        if (tsq_mv_key_lock(v, u, &t)) {
            if (first < 0) first = p;
        } else {
            const int64_t b = v.seg[u], e = b + v.cnt[u];
            if (chain > 0 && e - b >= chain) {
                int64_t i0 = tsq_mv_first_le(v.cts, b, e, t, &walked), found = -1;
                while (i0 < e && found < 0) {
                    for (int lane = 0; lane < 64 && found < 0; lane++)
                        if (tsq_mv_decides(v.types, i0 + lane, e)) found = i0 + lane;
                    i0 += 64;
                }
                res = found >= 0 ? tsq_mv_verdict(v.types, found) : -1;
            } else {
                res = tsq_mv_walk(v.cts, v.types, b, e, t, &walked);
            }
        }
        chosen[(size_t)p] = (int32_t)res;
    }
    // K21i .. K21l
    const int64_t M = P < lim ? P : lim;
    std::unique_ptr<int64_t[]> sel(new int64_t[(size_t)M]), selpos(new int64_t[(size_t)M]);
    int64_t T = 0;
    for (int64_t p = 0; p < P; p++)
        if (chosen[(size_t)p] >= 0) {
            if (T < M) {
                sel[(size_t)T] = chosen[(size_t)p];
                selpos[(size_t)T] = p;
            }
            T++;
        }
    const int64_t Tm = T < M ? T : M;
    const int64_t before = first >= 0 ? tsq_mv_lower_i64(selpos.get(), Tm, first) : Tm;
    if (first >= 0 && before < lim) {
        const int64_t r = tsq_mv_range_of(base.get(), R, first), rb = base[(size_t)r];
        const int64_t u = tsq_mv_key_at(rlo[(size_t)r], base[(size_t)r + 1] - rb, first - rb, desc);
        printf("R 17 %lld %d\n\n\n", (long long)before, v.lock[u]);
        return true;
    }
    printf("R 0 %lld -1\n", (long long)Tm);
    for (int64_t i = 0; i < Tm; i++) printf("%lld ", (long long)sel[(size_t)i]);
    printf("\n");
    for (long long r = 0; r < R; r++)
        printf("%lld ", (long long)(tsq_mv_lower_i64(selpos.get(), Tm, base[(size_t)r + 1]) - tsq_mv_lower_i64(selpos.get(), Tm, base[(size_t)r])));
    printf("\n");
    return true;
}

int main() {
    Store s;
    char op[8];
    while (scanf("%7s", op) == 1) {
        if (op[0] == 'S') {
            if (!read_store(s)) return 2;
        } else if (op[0] == 'Q') {
            if (!query(s)) return 2;
        } else {
            return 2;
        }
    }
    return 0;
}
