// Host build of tinysql_amd/csrc/tsq_memread_dp.h for tests/test_memread_cpu.py: the bound of every range end, the verdict of every
// point key, the exclusive scan of the position counts, position -> (range, entry), the keep rule, the ordinals and byte offsets,
// and the placement of every pair for an ascending and a descending scan — the steps tsq_memread.hip runs, one position at a time,
// over exactly sized heap arrays so that the sanitizers see any read past a key or an array; and the dirty-handle pass of a table.
// Reads from stdin (keys as hex, "-" for the empty string):
//   B <n>                 then n lines <op> <key> <value length>: the finished buffer, keys strictly ascending
//   S <desc> <n>          then n lines <start> <end>: a range scan
//   P <n>                 then n lines <key>: the point reads
//                         both print "S <pairs> <key bytes> <value bytes> <positions> <skipped dels>", "C" and the pairs of every range
//                         (points: of every key) on one line, then per pair in result order <entry> <key offset> <value offset>
//   D <table id>          prints "D <added> <deleted>", the added handles on one line, the deleted ones on the next;
//                         or "E invalid key"
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <memory>
#include <string>
#include <vector>

#include "../tinysql_amd/csrc/tsq_memread_dp.h"

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
// the exclusive scan the device runs over n values into n + 1 entries, in place
static void scan(int64_t* v, int64_t n) {
    int64_t run = 0;
    for (int64_t i = 0; i < n; i++) {
        const int64_t c = v[i];
        v[i] = run;
        run += c;
    }
    v[n] = run;
}

static char buf[1 << 16], buf2[1 << 16];

struct Buffer {
    std::unique_ptr<uint8_t[]> okeys, oops;
    std::unique_ptr<int64_t[]> okoff, ovoff;
    tsq_mr_buffer view() const {
        tsq_mr_buffer b;
        b.okeys = okeys.get(), b.okoff = okoff.get(), b.oops = oops.get(), b.ovoff = ovoff.get(), b.m = m;
        return b;
    }
    int64_t m = 0;
};

// everything behind the bounds: rlo [n], rcnt [n + 1] (the entries of every range)
static int run_positions(const tsq_mr_buffer& b, int64_t n, int64_t* rlo, int64_t* rcnt, int desc) {
    scan(rcnt, n);
    const int64_t positions = rcnt[n];
    std::unique_ptr<int64_t[]> entry(new int64_t[positions]), ord(new int64_t[positions + 1]), koff(new int64_t[positions + 1]), voff(new int64_t[positions + 1]);
    int64_t dels = 0;
    for (int64_t p = 0; p < positions; p++) {
        bool del;
        ord[p] = tsq_mr_mark(b, rlo, rcnt, n, p, &entry[p], &del, &koff[p], &voff[p]) ? 1 : 0;
        dels += del ? 1 : 0;
    }
    scan(ord.get(), positions);
    scan(koff.get(), positions);
    scan(voff.get(), positions);
    const int64_t pairs = ord[positions], kbytes = koff[positions], vbytes = voff[positions];
    printf("S %lld %lld %lld %lld %lld\nC", (long long)pairs, (long long)kbytes, (long long)vbytes, (long long)positions, (long long)dels);
    for (int64_t r = 0; r < n; r++) printf(" %lld", (long long)(ord[rcnt[r + 1]] - ord[rcnt[r]]));
    printf("\n");
    std::unique_ptr<int64_t[]> oe(new int64_t[pairs]), ok(new int64_t[pairs]), ov(new int64_t[pairs]);
    for (int64_t i = 0; i < pairs; i++) oe[i] = ok[i] = ov[i] = -1;
    for (int64_t p = 0; p < positions; p++) {
        if (ord[p + 1] == ord[p]) continue;
        const int64_t at = tsq_mr_place(ord[p], pairs, desc);
        if (at < 0 || at >= pairs || oe[at] != -1) {
            printf("pair %lld is placed at %lld\n", (long long)ord[p], (long long)at);
            return 1;
        }
        oe[at] = entry[p];
        ok[at] = tsq_mr_place_bytes(koff[p], koff[p + 1] - koff[p], kbytes, desc);
        ov[at] = tsq_mr_place_bytes(voff[p], voff[p + 1] - voff[p], vbytes, desc);
    }
    for (int64_t i = 0; i < pairs; i++) printf("%lld %lld %lld\n", (long long)oe[i], (long long)ok[i], (long long)ov[i]);
    return 0;
}

int main() {
    Buffer bf;
    char cmd[8];
    while (scanf("%7s", cmd) == 1) {
        if (cmd[0] == 'B') {
            long long n;
            if (scanf("%lld", &n) != 1) return 2;
            std::vector<uint8_t> kb, ops;
            std::vector<int64_t> ko(1, 0), vo(1, 0);
            for (long long i = 0; i < n; i++) {
                int op;
                long long vl;
                if (scanf("%d %65535s %lld", &op, buf, &vl) != 3) return 2;
                const std::vector<uint8_t> k = unhex(buf);
                kb.insert(kb.end(), k.begin(), k.end());
                ko.push_back((int64_t)kb.size());
                vo.push_back(vo.back() + vl);
                ops.push_back((uint8_t)op);
            }
            bf.okeys = exact(kb), bf.oops = exact(ops), bf.okoff = exact(ko), bf.ovoff = exact(vo), bf.m = n;
        } else if (cmd[0] == 'S') {
            int desc;
            long long n;
            if (scanf("%d %lld", &desc, &n) != 2) return 2;
            std::vector<uint8_t> rb;
            std::vector<int64_t> ro(1, 0);
            for (long long r = 0; r < n; r++) {
                if (scanf("%65535s %65535s", buf, buf2) != 2) return 2;
                for (const char* s : {buf, buf2}) {
                    const std::vector<uint8_t> k = unhex(s);
                    rb.insert(rb.end(), k.begin(), k.end());
                    ro.push_back((int64_t)rb.size());
                }
            }
            auto xb = exact(rb);
            auto xo = exact(ro);
            const tsq_mr_buffer b = bf.view();
            std::unique_ptr<int64_t[]> rlo(new int64_t[n]), rcnt(new int64_t[n + 1]);
            uint32_t err = 0;
            for (long long r = 0; r < n; r++) {  // (the device: one lane per bound, the even lane takes the odd one's answer)
                const int64_t lo = tsq_mr_range_bound(b, xb.get(), xo.get(), 2 * r, &err), hi = tsq_mr_range_bound(b, xb.get(), xo.get(), 2 * r + 1, &err);
                rlo[r] = lo;
                rcnt[r] = tsq_mr_range_count(lo, hi);
            }
            if (err) {
                printf("E offsets\n");
                continue;
            }
            if (run_positions(b, n, rlo.get(), rcnt.get(), desc)) return 1;
        } else if (cmd[0] == 'P') {
            long long n;
            if (scanf("%lld", &n) != 1) return 2;
            std::vector<uint8_t> kb;
            std::vector<int64_t> ko(1, 0);
            for (long long i = 0; i < n; i++) {
                if (scanf("%65535s", buf) != 1) return 2;
                const std::vector<uint8_t> k = unhex(buf);
                kb.insert(kb.end(), k.begin(), k.end());
                ko.push_back((int64_t)kb.size());
            }
            auto xb = exact(kb);
            auto xo = exact(ko);
            bool fixed = n > 0;
            for (long long i = 0; i < n && fixed; i++) fixed = ko[i + 1] - ko[i] == ko[1] - ko[0];
            const tsq_mr_buffer b = bf.view();
            std::unique_ptr<int64_t[]> rlo(new int64_t[n]), rcnt(new int64_t[n + 1]);
            uint32_t err = 0;
            for (long long i = 0; i < n; i++) {
                rlo[i] = tsq_mr_point(b, xb.get(), xo.get(), 0, (int64_t)kb.size(), i, &rcnt[i], &err);
                if (fixed) {  // keys of one length: once more through the fixed-length form, which must agree
                    int64_t c2;
                    if (tsq_mr_point(b, xb.get(), nullptr, ko[1] - ko[0], (int64_t)kb.size(), i, &c2, &err) != rlo[i] || c2 != rcnt[i]) {
                        printf("the fixed-length form differs at key %lld\n", i);
                        return 1;
                    }
                }
            }
            if (err) {
                printf("E offsets\n");
                continue;
            }
            if (run_positions(b, n, rlo.get(), rcnt.get(), 0)) return 1;
        } else if (cmd[0] == 'D') {
            long long tid;
            if (scanf("%lld", &tid) != 1) return 2;
            std::unique_ptr<uint8_t[]> rng(new uint8_t[22]);
            std::unique_ptr<int64_t[]> ro(new int64_t[3]);
            ro[0] = 0, ro[1] = 11, ro[2] = 22;
            tsq_mr_record_bound(tid, 0, rng.get());
            tsq_mr_record_bound(tid, 1, rng.get() + 11);
            const tsq_mr_buffer b = bf.view();
            uint32_t err = 0;
            const int64_t lo = tsq_mr_range_bound(b, rng.get(), ro.get(), 0, &err), hi = tsq_mr_range_bound(b, rng.get(), ro.get(), 1, &err);
            std::vector<long long> added, deleted;
            for (int64_t e = lo; e < lo + tsq_mr_range_count(lo, hi); e++) {
                int64_t h;
                const uint8_t op = tsq_mr_dirty_at(b, e, &h, &err);
                if (op == TSQ_MVCC_OP_PUT) added.push_back(h);
                else if (op == TSQ_MVCC_OP_DEL) deleted.push_back(h);
            }
            if (err) {
                printf("E invalid key\n");
                continue;
            }
            printf("D %zu %zu\n", added.size(), deleted.size());
            for (long long h : added) printf("%lld ", h);
            printf("\n");
            for (long long h : deleted) printf("%lld ", h);
            printf("\n");
        } else {
            return 2;
        }
    }
    return 0;
}
