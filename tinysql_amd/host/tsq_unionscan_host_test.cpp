// tsq_unionscan_host_test.cpp — the reference's dirty-transaction rows (executor/union_scan_test.go:26-48, :75-79) replayed through the
// C++ UnionScanExec of tsq_host.hpp on the GPU: table t (a int primary key, b int, index idx_b (b)); the child is a MockDataSource with
// the committed rows in scan order, the added rows are the transaction's in the same order.  The ORDER of the rows is the contract.
// Run by tests/test_unionscan_host_cpp_gpu.py; exit status 0 = every case passed.
#include <cstdio>
#include <map>

#include "tsq_host.hpp"

using namespace tsqhost;

static int g_fail = 0, g_pass = 0;
typedef std::pair<int64_t, int64_t> Row;  // (a, b)

static Chunk table(const std::vector<Row>& rows) {
    Chunk t(Schema(2, TSQ_I64));
    for (auto& r : rows) { t.columns[0].AppendInt64(r.first); t.columns[1].AppendInt64(r.second); }
    return t;
}
// scan order: table order (a), or idx_b order (b, a); desc reverses it
static std::vector<Row> in_order(std::map<int64_t, int64_t> rows, bool index, bool desc) {
    std::vector<Row> v(rows.begin(), rows.end());
    std::sort(v.begin(), v.end(), [&](const Row& x, const Row& y) { return index ? std::make_pair(x.second, x.first) < std::make_pair(y.second, y.first) : x < y; });
    if (desc) std::reverse(v.begin(), v.end());
    return v;
}
static void query(Context& ctx, const char* name, const std::map<int64_t, int64_t>& committed, const std::map<int64_t, int64_t>& mem, const DirtyTable& dirty,
                  bool index, bool desc, int chunk, const std::vector<Row>& want) {
    MockDataSource src(&ctx, table(in_order(committed, index, desc)), chunk);
    UnionScanExec us(&ctx, &src, &dirty, table(in_order(mem, index, desc)), index ? std::vector<int>{1} : std::vector<int>{}, 0, desc);
    us.maxChunkSize = chunk;
    std::vector<Row> got;
    for (Chunk& chk : Drain(&us))
        for (int64_t r = 0; r < chk.NumRows(); r++) got.push_back({chk.columns[0].GetInt64(r), chk.columns[1].GetInt64(r)});
    if (got == want) { g_pass++; printf("PASS %s (%zu rows)\n", name, got.size()); return; }
    g_fail++;
    printf("FAIL %s\n  got :", name);
    for (auto& r : got) printf(" [%lld %lld]", (long long)r.first, (long long)r.second);
    printf("\n");
}

int main() {
    if (tsq_device_count() <= 0) { printf("no HIP device: the host executors have no CPU fallback\n"); return 2; }
    Context ctx(0);
    std::map<int64_t, int64_t> committed = {{2, 3}, {4, 8}, {6, 8}}, mem;
    DirtyTable dirty;
    auto insert = [&](std::vector<Row> rows) { for (auto& r : rows) { mem[r.first] = r.second; dirty.AddRow(r.first); } };
    auto del = [&](std::vector<int64_t> hs) { for (auto h : hs) { mem.erase(h); dirty.DeleteRow(h); } };
    for (int chunk : {1, 2, 1024}) {
        mem.clear();
        dirty = DirtyTable();
        insert({{1, 5}, {3, 4}, {7, 6}});  // union_scan_test.go:29
        query(ctx, ":31 select * from t", committed, mem, dirty, false, false, chunk, {{1, 5}, {2, 3}, {3, 4}, {4, 8}, {6, 8}, {7, 6}});
        query(ctx, ":33 order by a desc", committed, mem, dirty, false, true, chunk, {{7, 6}, {6, 8}, {4, 8}, {3, 4}, {2, 3}, {1, 5}});
        query(ctx, ":34 order by b, a", committed, mem, dirty, true, false, chunk, {{2, 3}, {3, 4}, {1, 5}, {7, 6}, {4, 8}, {6, 8}});
        query(ctx, ":35 order by b desc, a desc", committed, mem, dirty, true, true, chunk, {{6, 8}, {4, 8}, {7, 6}, {1, 5}, {3, 4}, {2, 3}});
        del({2, 3});  // :38
        query(ctx, ":39 after delete", committed, mem, dirty, false, false, chunk, {{1, 5}, {4, 8}, {6, 8}, {7, 6}});
        query(ctx, ":40 after delete, desc", committed, mem, dirty, false, true, chunk, {{7, 6}, {6, 8}, {4, 8}, {1, 5}});
        query(ctx, ":41 after delete, order by b, a", committed, mem, dirty, true, false, chunk, {{1, 5}, {7, 6}, {4, 8}, {6, 8}});
        query(ctx, ":42 after delete, order by b desc, a desc", committed, mem, dirty, true, true, chunk, {{6, 8}, {4, 8}, {7, 6}, {1, 5}});
        insert({{2, 3}, {3, 4}});  // :44
        query(ctx, ":45 re-insert", committed, mem, dirty, false, false, chunk, {{1, 5}, {2, 3}, {3, 4}, {4, 8}, {6, 8}, {7, 6}});
        query(ctx, ":46 re-insert, desc", committed, mem, dirty, false, true, chunk, {{7, 6}, {6, 8}, {4, 8}, {3, 4}, {2, 3}, {1, 5}});
        query(ctx, ":47 re-insert, order by b, a", committed, mem, dirty, true, false, chunk, {{2, 3}, {3, 4}, {1, 5}, {7, 6}, {4, 8}, {6, 8}});
        query(ctx, ":48 re-insert, order by b desc, a desc", committed, mem, dirty, true, true, chunk, {{6, 8}, {4, 8}, {7, 6}, {1, 5}, {3, 4}, {2, 3}});
    }
    {   // :75-79 delete from t, then insert
        std::map<int64_t, int64_t> t2 = {{1, 1}, {2, 2}};
        mem.clear();
        dirty = DirtyTable();
        del({1, 2});
        query(ctx, ":76 delete from t", t2, mem, dirty, false, false, 1024, {});
        insert({{3, 1}});
        query(ctx, ":78 insert after delete", t2, mem, dirty, false, false, 1024, {{3, 1}});
        query(ctx, ":79 insert after delete, use index", t2, mem, dirty, true, false, 1024, {{3, 1}});
    }
    printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
