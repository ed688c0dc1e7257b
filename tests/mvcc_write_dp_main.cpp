// Host build of tinysql_amd/csrc/tsq_mvcc_write_dp.h for tests/test_mvcc_write_cpu.py: the request checks, the place of every request
// key in the store, the walk for the transaction's version — by one lane and in the wave form, emulated lane by lane — and the
// verdict with its plan, in the order k_mw_verdict of tsq_mvcc_write.hip runs them, over exactly sized heap arrays so that the
// sanitizers see any read past a key, a chain or an array.
// Reads from stdin (keys as hex, "-" for the empty string):
//   S <n> <n_locks>                       then n lines  <key> <commitTS> <startTS> <type>   (a store that passes the create checks)
//                                         and n_locks lines <key> <startTS> <op>
//                                         prints "U <keys of the universe>"
//   W <kind> <startTS> <commitTS> <chain> <q>   then q lines <key> <op> <value length>; kind: 0 prewrite, 1 commit, 2 rollback;
//                                         chain: the wave threshold (<= 0: never)
//                                         prints "E <error bits>", or "W <errors> <first error>" and q lines
//                                         <verdict> <info0> <info1> <flags> <type> <value lock> <version index> <lock index>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_mvcc_write_dp.h"

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
    std::unique_ptr<int32_t[]> ulen, useg, ucnt, ulock;
    int64_t n = 0, nl = 0, U = 0, key_bytes = 0;
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

static bool write_call(const Store& s) {
    int kind;
    unsigned long long start_ts, commit_ts;
    long long chain, q;
    if (scanf("%d %llu %llu %lld %lld", &kind, &start_ts, &commit_ts, &chain, &q) != 5 || q < 0 || !s.ok) return false;
    std::vector<uint8_t> kb, ops;
    std::vector<int64_t> koff(1, 0), voff(1, 0);
    for (long long i = 0; i < q; i++) {
        int op;
        long long vl;
        if (scanf("%65535s %d %lld", buf, &op, &vl) != 3) return false;
        const std::vector<uint8_t> k = unhex(buf);
        kb.insert(kb.end(), k.begin(), k.end());
        koff.push_back((int64_t)kb.size());
        ops.push_back((uint8_t)op);
        voff.push_back(voff.back() + vl);
    }
    const std::unique_ptr<uint8_t[]> rkeys = exact(kb), rops = exact(ops);
    const std::unique_ptr<int64_t[]> rkoff = exact(koff), rvoff = exact(voff);
    tsq_mw_store st;
    st.s.k.bytes = s.keys.get();
    st.s.k.beg = s.ubeg.get();
    st.s.k.len = s.ulen.get();
    st.s.k.n = s.U;
    st.s.seg = s.useg.get();
    st.s.cnt = s.ucnt.get();
    st.s.lock = s.ulock.get();
    st.s.cts = s.cts.get();
    st.s.types = s.types.get();
    st.s.l_start = s.lstart.get();
    st.s.l_op = s.lops.get();
    st.s.l_prim = nullptr;  // (no write reads a primary)
    st.s.l_poff = nullptr;
    st.sts = s.sts.get();
    st.n = s.n;
    st.lkeys = s.keys.get() + s.key_bytes;
    st.lkoff = s.lkoff.get();
    st.n_locks = s.nl;
    tsq_mw_req r;
    r.keys = rkeys.get();
    r.koff = rkoff.get();
    r.key_bytes = (int64_t)kb.size();
    r.q = q;
    r.ops = rops.get();
    r.voff = rvoff.get();
    r.value_bytes = voff.back();
    r.kind = kind;
    r.start_ts = start_ts;
    r.commit_ts = commit_ts;
    uint32_t bits = 0;
    for (long long i = 0; i < q; i++) bits |= tsq_mw_req_check(r, i);
    if (bits) {
        printf("E %u\n", bits);
        return true;
    }
    std::vector<tsq_mw_plan> plans((size_t)q);
    long long errors = 0, first = -1;
    for (long long i = 0; i < q; i++) {
        tsq_mw_place p;
        const int64_t b = r.koff[i];
        tsq_mw_locate(st, r.keys + b, r.koff[i + 1] - b, &p);
        int64_t found = -1;
        if (tsq_mw_needs_walk(st, r, p)) {
            if (chain > 0 && p.e - p.s >= chain) {
                for (int64_t j0 = p.s; j0 < p.e && found < 0; j0 += 64)
                    for (int lane = 0; lane < 64 && found < 0; lane++)
                        if (tsq_mw_is_start(st.sts, j0 + lane, p.e, r.start_ts)) found = j0 + lane;
            } else {
                found = tsq_mw_find_start(st.sts, p.s, p.e, r.start_ts);
            }
        }
        tsq_mw_decide(st, r, i, p, found, &plans[(size_t)i]);
        if (plans[(size_t)i].verdict >= TSQ_MVCC_V_LOCKED) {
            errors++;
            if (first < 0) first = i;
        }
    }
    printf("W %lld %lld\n", errors, first);
    for (const tsq_mw_plan& o : plans)
        printf("%d %llu %llu %d %d %d %d %d\n", (int)o.verdict, (unsigned long long)o.info0, (unsigned long long)o.info1, (int)o.flags, (int)o.vtype, o.vsrc, o.vpos,
               o.lpos);
    return true;
}

int main() {
    Store s;
    char op[8];
    while (scanf("%7s", op) == 1) {
        if (op[0] == 'S') {
            if (!read_store(s)) return 2;
        } else if (op[0] == 'W') {
            if (!write_call(s)) return 2;
        } else {
            return 2;
        }
    }
    return 0;
}
