"""The SEQUENTIAL model of the reference's duplicate-key handling: the yardstick of tsq_dupcheck_* and tsq_rows_equal.

A dict store (key bytes -> value, as kv.MemBuffer over the snapshot) and the two row loops of the reference, line by line:
  INSERT : InsertExec.exec -> addRecord per row (executor/insert.go:32-47) -> TableCommon.AddRecord -> addIndices
           (table/tables/tables.go:528-581): CheckHandleExists when PKIsHandle (:547-551), then index.Create of every writable index
           in order (:555-577; table/tables/index.go:194-261: a key with a NULL cell is not distinct and is written without a check),
           the first conflict ends the statement with kv.ErrKeyExists and the conflicting entry's handle.
  REPLACE: ReplaceExec.exec -> replaceRow per row (executor/replace.go:84-132) with removeRow (:53-81) and removeIndexRow (:140-161).
Keys are the oracle's encode_row_key / encode_index_keys, so key equality is the reference's (memcomparable encoding, prefix indexes —
the cell is truncated as tablecodec.TruncateIndexValues does — and NULL cells included).  If the parallel form the GPU runs and this
model ever disagree, the model wins.

Rows are tuples with None for NULL; integers are Python ints, doubles Python floats, strings bytes."""
import math

import numpy as np

from oracle import binding as orc
from tinysql_amd import _abi as abi
from tinysql_amd.chunk import Chunk, Column, StrColumn


class TableShape:
    """col_types: abi types of the table's columns; pk_col: the column that IS the handle (PKIsHandle) or None (the handle is
    _tidb_rowid); uniques: the unique indexes in WritableIndices order, each a list of (column, prefix length or None)."""

    def __init__(self, col_types, pk_col=None, uniques=(), table_id=41):
        self.col_types = list(col_types)
        self.pk_col = pk_col
        self.uniques = [[(c, p) for c, p in u] for u in uniques]
        self.table_id = table_id

    def n_streams(self):
        return (1 if self.pk_col is not None else 0) + len(self.uniques)

    def index_stream(self, i):
        return i + (1 if self.pk_col is not None else 0)


def column_of(tp, cells):
    if tp == abi.BYTES:
        return StrColumn(cells)
    nn = np.array([c is not None for c in cells], dtype=bool)
    return Column(tp, [0 if c is None else c for c in cells], nn)


def chunk_of(col_types, rows):
    return Chunk([column_of(tp, [r[c] for r in rows]) for c, tp in enumerate(col_types)])


_KEY_CACHE = {}


def index_keys(shape, i, rows):
    """the unique-index keys of `rows` for index i -> (list of key bytes, distinct flags); a key with a NULL cell is not distinct
    (index.go:105-123 GenIndexKey) and its bytes (written here WITHOUT the handle suffix) are never compared.  Keys come from the
    oracle; the cells -> key results are remembered, so that the thousands of small statements of the random tests ask it once per key."""
    cols = shape.uniques[i]
    types = tuple(shape.col_types[c] for c, _ in cols)
    cells = [tuple(r[c] if p is None or r[c] is None else r[c][:p] for c, p in cols) for r in rows]
    distinct = [all(v is not None for v in t) for t in cells]
    tags = [(shape.table_id, i, types, tuple(repr(v) for v in t)) for t in cells]
    missing = {}
    for tag, t in zip(tags, cells):
        if tag not in _KEY_CACHE:
            missing[tag] = t
    if missing:
        todo = list(missing.items())
        chk = Chunk([column_of(tp, [t[k] for _, t in todo]) for k, tp in enumerate(types)])
        keys, offs = orc.encode_index_keys(chk, shape.table_id, i + 1)
        raw = keys.tobytes()
        for k, (tag, _) in enumerate(todo):
            _KEY_CACHE[tag] = raw[offs[k]:offs[k + 1]]
    return [_KEY_CACHE[tag] for tag in tags], distinct


def datum_equal(a, b):
    """CompareDatum == 0 (types/datum.go:896-916, types/compare.go:104-123)"""
    if a is None or b is None:
        return a is None and b is None
    if isinstance(a, float) or isinstance(b, float):
        return not (math.isnan(a) or math.isnan(b)) and a == b
    return a == b


def equal_datums(ra, rb):
    return len(ra) == len(rb) and all(datum_equal(x, y) for x, y in zip(ra, rb))


class KeyExists(Exception):
    """kv.ErrKeyExists: statement row, stream, the handle of the entry that was there first"""

    def __init__(self, row, stream, dup_handle):
        Exception.__init__(self, "duplicate entry: row %d stream %d handle %d" % (row, stream, dup_handle))
        self.row, self.stream, self.dup_handle = row, stream, dup_handle


class Store:
    """the table in the KV store: record key -> (handle, row, origin) and, per unique index, distinct index key -> handle.
    origin: ('s', handle) for a row that was stored before the statement, ('b', statement row) for one the statement wrote."""

    def __init__(self, shape, stored=()):
        self.shape = shape
        self.rows = {}
        self.idx = [dict() for _ in shape.uniques]
        stored = list(stored)
        keys = [index_keys(shape, i, [r for _, r in stored]) for i in range(len(shape.uniques))]
        for k, (h, r) in enumerate(stored):
            self._put(h, r, ("s", h), [(ks[k], ds[k]) for ks, ds in keys])

    def _put(self, h, row, origin, ikeys):
        rk = orc.encode_row_key(self.shape.table_id, h)
        assert rk not in self.rows, "inconsistent store: handle twice"
        self.rows[rk] = (h, tuple(row), origin, ikeys)
        for i, (k, d) in enumerate(ikeys):
            if d:
                assert k not in self.idx[i], "inconsistent store: unique key twice"
                self.idx[i][k] = h

    def remove(self, h):
        """Table.RemoveRecord: the record and ALL its index entries (tables.go RemoveRecord -> removeRowIndices)"""
        rk = orc.encode_row_key(self.shape.table_id, h)
        _, _, origin, ikeys = self.rows.pop(rk)
        for i, (k, d) in enumerate(ikeys):
            if d:
                del self.idx[i][k]
        return origin

    def get(self, h):
        return self.rows.get(orc.encode_row_key(self.shape.table_id, h))

    def table(self):
        """{handle: row}"""
        return {h: r for h, r, _, _ in self.rows.values()}

    def sorted_handles(self):
        return sorted(h for h, _, _, _ in self.rows.values())

    def index_entries(self, i):
        """the distinct entries of index i in key order: [(key bytes, handle)]"""
        return sorted(self.idx[i].items())


def insert_stmt(shape, store, rows, rowid_base=0):
    """InsertExec.exec (executor/insert.go:32-47): rows in statement order; raises KeyExists at the first conflict (the statement's
    earlier rows are then rolled back by the caller: the store is left as it is HERE, callers that go on use a fresh one).
    -> (handles, new rowid_base)"""
    keys = [index_keys(shape, i, rows) for i in range(len(shape.uniques))]
    handles = []
    for r, row in enumerate(rows):
        if shape.pk_col is not None:
            h = row[shape.pk_col]
            if store.get(h) is not None:  # tables.go:547-551 CheckHandleExists
                raise KeyExists(r, 0, h)
        else:
            rowid_base += 1  # tables.go AddRecord: AllocHandle
            h = rowid_base
        for i in range(len(shape.uniques)):  # tables.go:555-577, in WritableIndices order
            k, d = keys[i][0][r], keys[i][1][r]
            if d and k in store.idx[i]:  # index.go:228-258: distinct -> Get; found -> ErrKeyExists with the stored handle
                raise KeyExists(r, shape.index_stream(i), store.idx[i][k])
        store._put(h, row, ("b", r), [(keys[i][0][r], keys[i][1][r]) for i in range(len(shape.uniques))])
        handles.append(h)
    return handles, rowid_base


def replace_stmt(shape, store, rows, rowid_base=0):
    """ReplaceExec.exec (executor/replace.go:163-196): replaceRow per row, in order.  Applies the statement to `store` and returns a dict:
    affected, added[r], handles[r] (None for an unchanged row), put[r] (added and still there at the end), removed_store (ascending
    handles of rows stored before the statement that it removed), n_removed_batch, rowid_base."""
    keys = [index_keys(shape, i, rows) for i in range(len(shape.uniques))]
    n = len(rows)
    affected = 0
    added = [False] * n
    handles = [None] * n
    removed_store, removed_batch = [], []

    def remove_row(h, new_row):  # replace.go:53-81 removeRow
        nonlocal affected
        old = store.get(h)
        assert old is not None, "can not be duplicated row, due to old row not found"  # :60-62
        if equal_datums(old[1], new_row):  # :66-73
            affected += 1
            return True
        origin = store.remove(h)  # :75
        (removed_store if origin[0] == "s" else removed_batch).append(origin[1])
        affected += 1  # :79
        return False

    for r, row in enumerate(rows):  # replace.go:84-132 replaceRow
        row = tuple(row)
        unchanged = False
        if shape.pk_col is not None:  # :90-109 r.handleKey != nil
            h = row[shape.pk_col]
            if store.get(h) is not None:
                unchanged = remove_row(h, row)
        while not unchanged:  # :112-124 keep on removing duplicated rows
            found = False
            for i in range(len(shape.uniques)):  # :140-161 removeIndexRow: the first unique key with a live entry
                k, d = keys[i][0][r], keys[i][1][r]
                if d and k in store.idx[i]:
                    unchanged = remove_row(store.idx[i][k], row)
                    found = True
                    break
            if not found:
                break
        if unchanged:
            continue
        if shape.pk_col is not None:  # :127 addRecord
            h = row[shape.pk_col]
        else:
            rowid_base += 1
            h = rowid_base
        store._put(h, row, ("b", r), [(keys[i][0][r], keys[i][1][r]) for i in range(len(shape.uniques))])
        affected += 1  # tables.go:496
        added[r] = True
        handles[r] = h
    gone = set(removed_batch)
    return dict(affected=affected, added=added, handles=handles, put=[added[r] and r not in gone for r in range(n)],
                removed_store=sorted(removed_store), n_removed_batch=len(removed_batch), rowid_base=rowid_base)
