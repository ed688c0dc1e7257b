"""A numpy restatement of IndexLookUpExecutor's double read (executor/distsql.go:237-637), written from the reference lines named
below.  Test infrastructure: every lookup test compares with it.

  cut_tasks      indexWorker.extractTaskHandles (:510-535): a task holds exactly batchSize handles (the last one: what is left);
                 batchSize starts at min(initBatchSize, maxBatchSize) (:328-330) and doubles after each FULL task up to
                 maxBatchSize (:530-533).
  lookup_task    the table worker (:601-637).  keep_order = False: the handles are sorted ascending as signed int64
                 (builder.go:940) and become point ranges (distsql/request_builder.go:161-180); the table scan returns the rows
                 that exist in handle order, a handle occurring twice gives its row twice, a missing handle nothing.
                 keep_order = True: the rows that exist in the task's index order (indexOrder, :538-546, 627-634).  PINNED
                 DEPARTURE: a handle occurring twice in one task yields its row at each occurrence's own position (the reference
                 puts both at the last occurrence's, indexOrder[h] = i overwrites); an index scan never yields a handle twice.
  The table's handles are in record-key order = signed int64 order of the raw 8 bytes (TestBigIntPK, distsql_test.go:102-108)."""
import numpy as np


def as_i64(values):
    """raw 8 bytes of a handle column: python ints beyond 2^63 - 1 (an unsigned PK) wrap to their signed image"""
    return np.array([int(v) & ((1 << 64) - 1) for v in values], dtype=np.uint64).view(np.int64)


def cut_tasks(n_handles, init_batch_size, max_batch_size):
    """-> [(first, last)] index ranges of the tasks over the index scan's handle sequence"""
    batch = min(int(init_batch_size), int(max_batch_size))
    assert batch >= 1
    out, at = [], 0
    while at < n_handles:
        n = min(batch, n_handles - at)
        out.append((at, at + n))
        at += n
        if n == batch:
            batch = min(batch * 2, int(max_batch_size))
    return out


def lookup_task(table_handles, handles, keep_order):
    """-> (rows, handles_out): table row ordinals of the emitted rows and their handles, in emission order"""
    table = np.asarray(table_handles, dtype=np.int64)
    hs = np.asarray(handles, dtype=np.int64)
    if not keep_order:
        hs = np.sort(hs, kind="stable")
    if table.size == 0 or hs.size == 0:
        return np.zeros(0, np.int64), np.zeros(0, np.int64)
    pos = np.searchsorted(table, hs, side="left")
    hit = pos < table.size
    hit[hit] = table[pos[hit]] == hs[hit]
    return pos[hit].astype(np.int64), hs[hit]


def index_lookup(table_handles, index_handles, keep_order, init_batch_size, max_batch_size, row_filter=None):
    """the reader's output as table row ordinals: tasks are emitted in order (resultCh); row_filter(rows) -> bool mask is the
    table-side plan (tblPlans), which drops rows without disturbing their order"""
    index_handles = np.asarray(index_handles, dtype=np.int64)
    out = []
    for lo, hi in cut_tasks(index_handles.size, init_batch_size, max_batch_size):
        rows, _ = lookup_task(table_handles, index_handles[lo:hi], keep_order)
        if row_filter is not None and rows.size:
            rows = rows[np.asarray(row_filter(rows), dtype=bool)]
        out.append(rows)
    return np.concatenate(out) if out else np.zeros(0, np.int64)


# ---------------------------------------------------------------- the golden cases (tests/golden/index_lookup_cases.json)
def load_cases():
    import json
    import os
    with open(os.path.join(os.path.dirname(os.path.abspath(__file__)), "golden", "index_lookup_cases.json")) as f:
        return json.load(f)["cases"]


OPS = {"gt": lambda a, b: a > b, "ge": lambda a, b: a >= b, "lt": lambda a, b: a < b, "le": lambda a, b: a <= b, "eq": lambda a, b: a == b}


def case_table(case):
    """-> (handles sorted as signed int64, rows in that order): the table as its record keys order it"""
    hs = as_i64([r["handle"] for r in case["rows"]])
    order = np.argsort(hs, kind="stable")
    return hs[order], [tuple(case["rows"][i]["values"]) for i in order]


def run_case(case, init_batch_size=None, max_batch_size=None):
    """the reader's rows of a golden case under the restatement"""
    hs, rows = case_table(case)
    cond = case.get("tbl_condition")
    flt = None
    if cond:
        flt = lambda ords: [OPS[cond["op"]](rows[i][cond["col"]], cond["value"]) for i in ords]  # noqa: E731
    size = max_batch_size or case["index_lookup_size"]
    ords = index_lookup(hs, as_i64(case["index_handles"]), case["keep_order"], init_batch_size or case["init_batch_size"], size, flt)
    return [list(rows[i]) for i in ords]


def apply_parent(case, rows):
    """what the plan above the reader does with its rows (TopN / Limit / Projection), to reach the reference's query result"""
    p = case.get("parent") or {}
    rows = [list(r) for r in rows]
    if "topn" in p:
        rows.sort(key=lambda r: r[p["topn"]["col"]], reverse=bool(p["topn"]["desc"]))
    if "count" in p:
        rows = rows[p.get("offset", 0):p.get("offset", 0) + p["count"]]
    if "project" in p:
        rows = [[r[c] for c in p["project"]] for r in rows]
    return rows
