// tsq_lookup_host_test.cpp — the reference's double-read cases (executor/executor_test.go:551-566, 710-720, 762-766, 1026-1029,
// executor/distsql_test.go:102-108, 147-160) replayed through the C++ IndexLookUpExecutor of tsq_host.hpp on the GPU.  Every table is
// built as its KV pairs (stored rows by tsq_rowcodec_encode, record keys by tsq_rowkeys_encode, index entries by tsq_indexkeys_encode);
// the index side is a mocktikv::indexScanExec over the entries the query's index scan delivers, optionally under limitExec.  The rows
// are compared in order.  Run by tests/test_lookup_host_cpp_gpu.py; exit status 0 = every case passed.
#include <cstdio>

#include "tsq_host.hpp"

using namespace tsqhost;

static int g_fail = 0, g_pass = 0;
typedef std::vector<int64_t> Row;

struct Table {
    std::vector<int64_t> handles;  // record-key order (signed)
    std::vector<Row> rows;         // the scan's columns of every row, in that order
    mocktikv::Pairs pairs;
    std::vector<mocktikv::ColInfo> cols;
};
// columns 0 .. ncols-1 under ids 1 .. ncols; pk >= 0: that column is the integer primary key (its value is the handle and is not
// stored), else the handles are the row ids 1, 2, ... in insert order
static Table make_table(Context& ctx, int ncols, int pk, bool pkUnsigned, std::vector<Row> inserted) {
    Table t;
    std::vector<std::pair<int64_t, Row>> byHandle;
    for (size_t i = 0; i < inserted.size(); i++) byHandle.push_back({pk >= 0 ? inserted[i][(size_t)pk] : (int64_t)i + 1, inserted[i]});
    std::sort(byHandle.begin(), byHandle.end());
    Schema stored;
    std::vector<int64_t> ids;
    for (int c = 0; c < ncols; c++) {
        t.cols.push_back({c + 1, c == pk && pkUnsigned ? TSQ_U64 : TSQ_I64, c == pk});
        if (c != pk) { stored.push_back(TSQ_I64); ids.push_back(c + 1); }
    }
    Chunk chk(stored);
    for (auto& hr : byHandle) {
        t.handles.push_back(hr.first);
        t.rows.push_back(hr.second);
        int k = 0;
        for (int c = 0; c < ncols; c++)
            if (c != pk) chk.columns[(size_t)k++].AppendInt64(hr.second[(size_t)c]);
    }
    const int64_t n = (int64_t)t.handles.size();
    auto v = chk.Views();
    int64_t need = 0;
    const tsq_status st = tsq_rowcodec_encode(ctx.h, v.data(), (int32_t)v.size(), ids.data(), nullptr, n, nullptr, 0, 0, nullptr, &need);
    if (st != TSQ_OK && st != TSQ_ERR_INVALID) check(st, ctx.h);
    t.pairs.values.resize((size_t)need + 8);
    t.pairs.valueOffsets.resize((size_t)n + 1);
    check(tsq_rowcodec_encode(ctx.h, v.data(), (int32_t)v.size(), ids.data(), nullptr, n, t.pairs.values.data(), need, 0, t.pairs.valueOffsets.data(), &need), ctx.h);
    t.pairs.values.resize((size_t)need);
    t.pairs.keys = EncodeRowKeysWithHandles(&ctx, 45, t.handles);
    return t;
}
// the index entries of the rows with the given handles, in the order given (what the query's index scan delivers)
static mocktikv::IndexPairs make_index(Context& ctx, const Table& t, const std::vector<int>& indexCols, bool unique, const std::vector<int64_t>& delivered) {
    Chunk chk(Schema(indexCols.size(), TSQ_I64));
    for (size_t c = 0; c < indexCols.size(); c++) chk.columns[c].type = t.cols[(size_t)indexCols[c]].type;
    for (int64_t h : delivered) {
        const size_t r = (size_t)(std::lower_bound(t.handles.begin(), t.handles.end(), h) - t.handles.begin());
        for (size_t c = 0; c < indexCols.size(); c++) chk.columns[c].AppendInt64(t.rows[r][(size_t)indexCols[c]]);
    }
    const int64_t n = (int64_t)delivered.size();
    mocktikv::IndexPairs p;
    p.keyOffsets.assign((size_t)n + 1, 0);
    p.valueOffsets.assign((size_t)n + 1, 0);
    p.values.resize((size_t)n * 8 + 8);
    std::vector<uint8_t> distinct((size_t)n + 1);
    auto v = chk.Views();
    int64_t need = 0;
    p.keys.resize(8);
    const tsq_status st = tsq_indexkeys_encode(ctx.h, 45, 2, unique ? TSQ_IDX_UNIQUE : 0, v.data(), (int32_t)v.size(), nullptr, nullptr, delivered.data(), n, 0, nullptr, 0,
                                               p.keyOffsets.data(), p.values.data(), p.valueOffsets.data(), distinct.data(), &need);
    if (st != TSQ_OK && st != TSQ_ERR_INVALID) check(st, ctx.h);
    p.keys.resize((size_t)need + 8);
    check(tsq_indexkeys_encode(ctx.h, 45, 2, unique ? TSQ_IDX_UNIQUE : 0, v.data(), (int32_t)v.size(), nullptr, nullptr, delivered.data(), n, 0, p.keys.data(), need,
                               p.keyOffsets.data(), p.values.data(), p.valueOffsets.data(), distinct.data(), &need), ctx.h);
    p.keys.resize((size_t)need);
    p.values.resize((size_t)p.valueOffsets[(size_t)n]);
    return p;
}

struct Query {
    const char* name;
    std::vector<int> indexCols;
    bool unique;
    std::vector<int64_t> delivered;  // handles in the order the index side hands them out
    int64_t indexLimit;              // a limitExec above the index scan (< 0: none)
    bool keepOrder;
    std::vector<Expression> tblConds;
    std::vector<Row> want;           // the reader's rows, in order
};

static void run(Context& ctx, const Table& t, const Query& q, int init, int maxBatch, const std::vector<int64_t>* wantTasks = nullptr) {
    mocktikv::IndexPairs ip = make_index(ctx, t, q.indexCols, q.unique, q.delivered);
    Schema itypes;
    for (int c : q.indexCols) itypes.push_back(t.cols[(size_t)c].type);
    bool pkU = false;
    for (auto& c : t.cols) pkU = pkU || (c.IsPKHandle && c.type == TSQ_U64);
    itypes.push_back(pkU ? TSQ_U64 : TSQ_I64);
    mocktikv::indexScanExec scan(&ctx, itypes, (int)q.indexCols.size(), pkU ? mocktikv::PrimaryKeyIsUnsigned : mocktikv::PrimaryKeyIsSigned, &ip);
    scan.maxChunkSize = 2;  // tasks are cut across the index side's chunks
    mocktikv::limitExec lim(&ctx, &scan, (uint64_t)(q.indexLimit < 0 ? 0 : q.indexLimit));
    lim.maxChunkSize = 2;
    Executor* idx = q.indexLimit < 0 ? (Executor*)&scan : (Executor*)&lim;
    IndexLookUpExecutor e(&ctx, idx, &t.pairs, t.cols, q.tblConds, q.keepOrder, init, maxBatch);
    std::vector<Row> got;
    std::vector<Chunk> chunks = Drain(&e);
    for (Chunk& chk : chunks)
        for (int64_t r = 0; r < chk.NumRows(); r++) {
            Row row;
            for (auto& c : chk.columns) row.push_back(c.GetInt64(r));
            got.push_back(row);
        }
    bool ok = got == q.want;
    if (ok && wantTasks) ok = e.taskSizes == *wantTasks;
    char label[256];
    snprintf(label, sizeof label, "%s [batch %d..%d]", q.name, init, maxBatch);
    if (ok) { g_pass++; printf("PASS %s (%zu rows)\n", label, got.size()); return; }
    g_fail++;
    printf("FAIL %s\n  got :", label);
    for (auto& r : got) {
        printf(" [");
        for (auto v : r) printf(" %lld", (long long)v);
        printf(" ]");
    }
    printf("\n  tasks:");
    for (auto s : e.taskSizes) printf(" %lld", (long long)s);
    printf("\n");
}
// a keep-order query gives the same rows for every cut of its handles
static void run_cuts(Context& ctx, const Table& t, const Query& q) {
    run(ctx, t, q, 1024, 20000);
    if (!q.keepOrder) return;
    run(ctx, t, q, 1, 3);
    run(ctx, t, q, 2, 2);
    run(ctx, t, q, 1, 1 << 20);
}

int main() {
    if (tsq_device_count() <= 0) { printf("no HIP device: the host executors have no CPU fallback\n"); return 2; }
    Context ctx(0);
    {   // executor_test.go:551-557: t(a int primary key, b, c, index idx(b)); use index(idx) order by a desc limit 1 — the TopN runs on the index side
        Table t = make_table(ctx, 3, 0, false, {{1, 3, 1}, {2, 2, 2}, {3, 1, 3}});
        run_cuts(ctx, t, {":557 double read under a TopN", {1}, false, {3}, -1, false, {}, {{3, 1, 3}}});
    }
    {   // :559-566: t(a, b, key b (b)), IndexLookupSize = 3, rows (i, 10 - i): select a from t use index(b) order by b
        std::vector<Row> ins, want;
        for (int64_t i = 0; i < 10; i++) ins.push_back({i, 10 - i});
        for (int64_t k = 0; k < 10; k++) want.push_back({9 - k, 1 + k});
        Table t = make_table(ctx, 2, -1, false, ins);
        Query q{":566 keep order, IndexLookupSize = 3", {1}, false, {10, 9, 8, 7, 6, 5, 4, 3, 2, 1}, -1, true, {}, want};
        const std::vector<int64_t> tasks = {3, 3, 3, 1};
        run(ctx, t, q, 1024, 3, &tasks);
        run_cuts(ctx, t, q);
    }
    {   // :710-720: t(a int unique, b); select * from t order by a limit 3 — the limit is pushed to the index side
        Table t = make_table(ctx, 2, -1, false, {{5, 0}, {4, 0}, {3, 0}, {2, 0}, {1, 0}, {0, 0}});
        run_cuts(ctx, t, {":720 unique index order, limit 3", {0}, true, {6, 5, 4, 3, 2, 1}, 3, true, {}, {{0, 0}, {1, 0}, {2, 0}}});
    }
    {   // :762-766: t(a int primary key, b, c, index(c)); where c >= 2 order by b desc limit 1: the reader's rows come in handle order
        Table t = make_table(ctx, 3, 0, false, {{1, 1, 1}, {2, 2, 2}, {4, 4, 4}, {3, 3, 3}, {5, 5, 5}});
        run_cuts(ctx, t, {":766 double read and top n", {2}, false, {2, 3, 4, 5}, -1, false, {}, {{2, 2, 2}, {3, 3, 3}, {4, 4, 4}, {5, 5, 5}}});
    }
    {   // :1026-1029: t(a, b, index idx(a)), rows (3,3) (1,1) (2,2); use index(idx) order by a
        Table t = make_table(ctx, 2, -1, false, {{3, 3}, {1, 1}, {2, 2}});
        run_cuts(ctx, t, {":1029 second test double read", {0}, false, {2, 3, 1}, -1, true, {}, {{1, 1}, {2, 2}, {3, 3}}});
    }
    {   // distsql_test.go:102-108: t(a bigint unsigned primary key, b, c, index idx(a, b)); use index(idx) order by a
        const int64_t big = 9223372036854775807LL;
        Table t = make_table(ctx, 3, 0, true, {{1, 1, 1}, {big, 2, 2}});
        run_cuts(ctx, t, {"distsql :107 unsigned PK at 2^63-1", {0, 1}, false, {1, big}, -1, true, {}, {{1, 1, 1}, {big, 2, 2}}});
    }
    {   // distsql_test.go:147-160: tbl(a, b, c, key idx_b_c(b, c)), rows (i, i, i): the limit (offset + count) below the lookup
        Table t = make_table(ctx, 3, -1, false, {{1, 1, 1}, {2, 2, 2}, {3, 3, 3}, {4, 4, 4}, {5, 5, 5}});
        auto rows = [](std::vector<int64_t> hs) { std::vector<Row> r; for (auto h : hs) r.push_back({h, h, h}); return r; };
        run_cuts(ctx, t, {"distsql :153 b > 1 limit 2,1", {1, 2}, false, {2, 3, 4, 5}, 3, false, {}, rows({2, 3, 4})});
        run_cuts(ctx, t, {"distsql :154 b > 4 limit 2,1", {1, 2}, false, {5}, 3, false, {}, rows({5})});
        run_cuts(ctx, t, {"distsql :155 b > 3 limit 2,1", {1, 2}, false, {4, 5}, 3, false, {}, rows({4, 5})});
        run_cuts(ctx, t, {"distsql :156 b > 2 limit 2,1", {1, 2}, false, {3, 4, 5}, 3, false, {}, rows({3, 4, 5})});
        run_cuts(ctx, t, {"distsql :157 b > 1 limit 1", {1, 2}, false, {2, 3, 4, 5}, 1, false, {}, rows({2})});
        run_cuts(ctx, t, {"distsql :158 b > 1 order by b desc limit 2,1", {1, 2}, false, {5, 4, 3, 2}, 3, true, {}, rows({5, 4, 3})});
        // c > 1 as a table-side condition: the limit stays above the lookup
        run_cuts(ctx, t, {"distsql :159 b > 1 and c > 1", {1, 2}, false, {2, 3, 4, 5}, -1, false, {Func("gt", {Col(2, TSQ_I64), Int(1)})}, rows({2, 3, 4, 5})});
        run_cuts(ctx, t, {"table-side condition c > 3, keep order, descending index", {1, 2}, false, {5, 4, 3, 2, 1}, -1, true, {Func("gt", {Col(2, TSQ_I64), Int(3)})}, rows({5, 4})});
    }
    printf("%d passed, %d failed\n", g_pass, g_fail);
    return g_fail ? 1 : 0;
}
