// Host build of tinysql_amd/csrc/tsq_mvcc_maint_dp.h for tests/test_mvcc_maint_cpu.py: a key range as bounds in the three index spaces
// of a store, ScanLock's test, ResolveLock's decision and placement per lock, GC's two indices per key — by one lane and in the wave
// form, emulated lane by lane — and its drop test per entry, in the order the kernels of tsq_mvcc_maint.hip run them, over exactly
// sized heap arrays so that the sanitizers see any read past a key, a chain or an array.
// Reads from stdin (keys as hex, "-" for the empty string):
//   S <n> <n_locks>                 the store, as tests/mvcc_write_dp_main.cpp takes it; prints "U <keys of the universe>"
//   R <start> <end>                 prints "R <u0> <u1> <e0> <e1> <l0> <l1>"
//   L <start> <end> <max_ts>        prints "L <hits>" and one line with the hits' lock indexes
//   V <start> <end> <T>             then T lines <start_ts> <commit_ts>, ascending by start_ts; prints "V <l0> <q>" and q lines
//                                   <flags> <type> <value lock> <version index> <lock index> <commitTS>
//   G <start> <end> <safe_point> <chain>   chain: the wave threshold (<= 0: never); prints "G <refusing locks> <first or -1>", then
//                                   "D <drops>" and one line with the dropped entries' indexes
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_mvcc_maint_dp.h"

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
    std::unique_ptr<uint8_t[]> keys, types, lops;
    std::unique_ptr<int64_t[]> koff, lkoff, ubeg;
    std::unique_ptr<uint64_t[]> cts, sts, lstart;
    std::unique_ptr<int32_t[]> ulen, useg, ucnt, ulock, ord, seg;
    int64_t n = 0, nl = 0, U = 0, K = 0, key_bytes = 0;
    bool ok = false;
};

static char buf[1 << 16];

static bool read_store(Store& s) {
    long long n, nl;
    if (scanf("%lld %lld", &n, &nl) != 2 || n < 0 || nl < 0) return false;
    std::vector<std::vector<uint8_t>> vk, lk;
    std::vector<uint8_t> kb, lkb, types, lops;
    std::vector<int64_t> koff(1, 0), lkoff(1, 0);
    std::vector<uint64_t> cts, sts, lstart;
    for (long long i = 0; i < n; i++) {
        unsigned long long c, st;
        int t;
        if (scanf("%65535s %llu %llu %d", buf, &c, &st, &t) != 4) return false;
        vk.push_back(unhex(buf));
        kb.insert(kb.end(), vk.back().begin(), vk.back().end());
        koff.push_back((int64_t)kb.size());
        cts.push_back(c);
        sts.push_back(st);
        types.push_back((uint8_t)t);
    }
    for (long long j = 0; j < nl; j++) {
        unsigned long long st;
        int op;
        if (scanf("%65535s %llu %d", buf, &st, &op) != 3) return false;
        lk.push_back(unhex(buf));
        lkb.insert(lkb.end(), lk.back().begin(), lk.back().end());
        lkoff.push_back((int64_t)lkb.size());
        lstart.push_back(st);
        lops.push_back((uint8_t)op);
    }
    s.key_bytes = (int64_t)kb.size();
    // the key universe, by a merge of the two sorted lists (the create kernels of tsq_mvcc.hip build the same; tests/mvcc_dp_main.cpp
    // holds them to the model)
    std::vector<int64_t> ubeg;
    std::vector<int32_t> ulen, useg, ucnt, ulock;
    long long i = 0, j = 0;
    while (i < n || j < nl) {
        int c = 0;
        if (i >= n) c = 1;
        else if (j >= nl) c = -1;
        else c = vk[(size_t)i] < lk[(size_t)j] ? -1 : (vk[(size_t)i] == lk[(size_t)j] ? 0 : 1);
        if (c <= 0) {
            long long e = i;
            while (e < n && vk[(size_t)e] == vk[(size_t)i]) e++;
            ubeg.push_back(koff[(size_t)i]);
            ulen.push_back((int32_t)vk[(size_t)i].size());
            useg.push_back((int32_t)i);
            ucnt.push_back((int32_t)(e - i));
            ulock.push_back(c == 0 ? (int32_t)j : -1);
            if (c == 0) j++;
            i = e;
        } else {
            ubeg.push_back(s.key_bytes + lkoff[(size_t)j]);
            ulen.push_back((int32_t)lk[(size_t)j].size());
            useg.push_back((int32_t)i);  // where its versions would go
            ucnt.push_back(0);
            ulock.push_back((int32_t)j);
            j++;
        }
    }
    // the ordinal of every entry among the K keys with versions and their K + 1 segment starts (k_mv_ordinals of tsq_mvcc.hip)
    std::vector<int32_t> ord, seg;
    for (long long e = 0; e < n; e++) {
        if (e == 0 || vk[(size_t)e] != vk[(size_t)e - 1]) seg.push_back((int32_t)e);
        ord.push_back((int32_t)seg.size() - 1);
    }
    s.K = (int64_t)seg.size();
    seg.push_back((int32_t)n);
    s.ord = exact(ord);
    s.seg = exact(seg);
    kb.insert(kb.end(), lkb.begin(), lkb.end());  // the store's keys, then the locks' keys
    s.keys = exact(kb);
    s.types = exact(types);
    s.lops = exact(lops);
    s.koff = exact(koff);
    s.lkoff = exact(lkoff);
    s.cts = exact(cts);
    s.sts = exact(sts);
    s.lstart = exact(lstart);
    s.ubeg = exact(ubeg);
    s.ulen = exact(ulen);
    s.useg = exact(useg);
    s.ucnt = exact(ucnt);
    s.ulock = exact(ulock);
    s.n = n;
    s.nl = nl;
    s.U = (int64_t)ubeg.size();
    s.ok = true;
    printf("U %lld\n", (long long)s.U);
    return true;
}


static void view(const Store& s, tsq_mw_store* st) {
    st->s.k.bytes = s.keys.get();
    st->s.k.beg = s.ubeg.get();
    st->s.k.len = s.ulen.get();
    st->s.k.n = s.U;
    st->s.seg = s.useg.get();
    st->s.cnt = s.ucnt.get();
    st->s.lock = s.ulock.get();
    st->s.cts = s.cts.get();
    st->s.types = s.types.get();
    st->s.l_start = s.lstart.get();
    st->s.l_op = s.lops.get();
    st->s.l_prim = nullptr;  // (no range call reads a primary through the view)
    st->s.l_poff = nullptr;
    st->sts = s.sts.get();
    st->n = s.n;
    st->lkeys = s.keys.get() + s.key_bytes;
    st->lkoff = s.lkoff.get();
    st->n_locks = s.nl;
}

static char buf2[1 << 16];

static bool range_of(const Store& s, tsq_mw_store* st, tsq_mm_bounds* b) {
    if (!s.ok || scanf("%65535s %65535s", buf, buf2) != 2) return false;
    const std::vector<uint8_t> a = unhex(buf), e = unhex(buf2);
    const std::unique_ptr<uint8_t[]> pa = exact(a), pe = exact(e);
    view(s, st);
    tsq_mm_range(*st, pa.get(), (int64_t)a.size(), pe.get(), (int64_t)e.size(), b);
    return b->u0 >= 0 && b->u1 >= b->u0 && b->u1 <= s.U && b->e0 >= 0 && b->e1 >= b->e0 && b->e1 <= s.n && b->l0 >= 0 && b->l1 >= b->l0 && b->l1 <= s.nl;
}

static bool gc_call(const Store& s) {
    tsq_mw_store st;
    tsq_mm_bounds b;
    unsigned long long safe;
    long long chain;
    if (!range_of(s, &st, &b) || scanf("%llu %lld", &safe, &chain) != 2) return false;
    long long nerr = 0, first = -1;
    for (int64_t j = b.l0; j < b.l1; j++)
        if (tsq_mm_lock_le(st.s.l_start, j, safe)) {
            nerr++;
            if (first < 0) first = j;
        }
    printf("G %lld %lld\n", nerr, first);
    const int64_t k0 = b.e0 < s.n ? s.ord[b.e0] : s.K, k1 = b.e1 < s.n ? s.ord[b.e1] : s.K;
    if (k1 < k0 || k1 > s.K) return false;
    const int64_t nk = k1 - k0;
    std::vector<int32_t> vlo((size_t)nk), vkeep((size_t)nk);
    const std::unique_ptr<int32_t[]> glo = exact(vlo), gkeep = exact(vkeep);
    for (int64_t i = 0; i < nk; i++) {
        const int64_t k = k0 + i, cs = s.seg[k], ce = s.seg[k + 1];
        const int64_t lo = tsq_mm_gc_lo(st.s.cts, cs, ce, safe);
        int64_t f = -1;
        if (chain > 0 && ce - cs >= chain) {
            for (int64_t j0 = lo; j0 < ce && f < 0; j0 += 64)
                for (int lane = 0; lane < 64 && f < 0; lane++)
                    if (tsq_mv_decides(st.s.types, j0 + lane, ce)) f = j0 + lane;
        } else {
            f = tsq_mm_gc_first(st.s.types, lo, ce);
        }
        glo[i] = (int32_t)lo;
        gkeep[i] = (int32_t)tsq_mm_gc_keeper(st.s.types, f);
    }
    std::vector<long long> drops;
    for (int64_t p = b.e0; p < b.e1; p++) {
        const int64_t k = (int64_t)s.ord[p] - k0;
        if (k < 0 || k >= nk) return false;
        if (tsq_mm_gc_drops(p, glo[k], gkeep[k])) drops.push_back(p);
    }
    printf("D %zu\n", drops.size());
    for (long long p : drops) printf("%lld ", p);
    printf("\n");
    return true;
}

int main() {
    Store s;
    char op[8];
    while (scanf("%7s", op) == 1) {
        tsq_mw_store st;
        tsq_mm_bounds b;
        if (op[0] == 'S') {
            if (!read_store(s)) return 2;
        } else if (op[0] == 'R') {
            if (!range_of(s, &st, &b)) return 2;
            printf("R %lld %lld %lld %lld %lld %lld\n", (long long)b.u0, (long long)b.u1, (long long)b.e0, (long long)b.e1, (long long)b.l0, (long long)b.l1);
        } else if (op[0] == 'L') {
            unsigned long long max_ts;
            if (!range_of(s, &st, &b) || scanf("%llu", &max_ts) != 1) return 2;
            std::vector<long long> hits;
            for (int64_t j = b.l0; j < b.l1; j++)
                if (tsq_mm_lock_le(st.s.l_start, j, max_ts)) hits.push_back(j);
            printf("L %zu\n", hits.size());
            for (long long j : hits) printf("%lld ", j);
            printf("\n");
        } else if (op[0] == 'V') {
            long long T;
            if (!range_of(s, &st, &b) || scanf("%lld", &T) != 1 || T < 0) return 2;
            std::vector<uint64_t> ts, tc;
            for (long long i = 0; i < T; i++) {
                unsigned long long x, y;
                if (scanf("%llu %llu", &x, &y) != 2) return 2;
                ts.push_back(x);
                tc.push_back(y);
            }
            const std::unique_ptr<uint64_t[]> pts = exact(ts), ptc = exact(tc);
            printf("V %lld %lld\n", (long long)b.l0, (long long)(b.l1 - b.l0));
            for (int64_t j = b.l0; j < b.l1; j++) {
                tsq_mw_plan o;
                tsq_mm_resolve(st, j, pts.get(), ptc.get(), T, &o);
                printf("%d %d %d %d %d %llu\n", (int)o.flags, (int)o.vtype, o.vsrc, o.vpos, o.lpos, (unsigned long long)o.vcts);
            }
        } else if (op[0] == 'G') {
            if (!gc_call(s)) return 2;
        } else {
            return 2;
        }
    }
    return 0;
}
