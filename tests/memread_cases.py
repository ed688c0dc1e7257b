"""What the CPU and the GPU tests of the mem readers share: tests/golden/memread_cases.json turned into KV pairs (the oracle's row and
index-key encoders), the steps of a case replayed into any buffer with Set / Delete (the dict model, a kv.MemBuffer), and per read
its kv ranges, the reader's schema, the union scan's order, the committed rows in scan order and the conditions as a Python predicate
and as expressions."""
import functools
import json
import os

import numpy as np

from tests import memread_ref as R
from tests.unionscan_ref import UnionScanRef
from tinysql_amd import _abi as abi
from tinysql_amd import expression as E
from tinysql_amd import rowcodec as RC
from tinysql_amd.chunk import Chunk, Column, StrColumn

ROOT = os.path.dirname(os.path.dirname(os.path.abspath(__file__)))
PK_SIGNED, PK_UNSIGNED = 1, 2  # tablecodec.PrimaryKeyIsSigned / PrimaryKeyIsUnsigned


def golden():
    return json.load(open(os.path.join(ROOT, "tests", "golden", "memread_cases.json")))["cases"]


def cell_column(tp, values):
    if tp == abi.BYTES:
        return StrColumn(values)
    nn = np.array([v is not None for v in values], dtype=bool)
    data = np.array([0 if v is None else v for v in values], dtype=np.uint64 if tp == abi.U64 else np.int64)
    return Column(tp, data, None if nn.all() else nn)


def edge_ranges(keys):
    """bounds equal to a stored key, proper prefixes, extensions by 0x00, the empty bounds, start >= end, overlapping and identical ranges"""
    ks = sorted(keys)
    pick = ks[::max(1, len(ks) // 12)] + ks[-1:]
    rs = [(b"", b""), (b"", ks[0]), (ks[-1], b""), (ks[0], ks[-1]), (ks[-1], ks[0]), (ks[0], ks[0])]
    for k in pick:
        rs += [(k, k + b"\x00"), (k + b"\x00", b""), (b"", k[:-1]), (k[:-1], k), (k[:max(1, len(k) // 2)], k + b"\x00\x00"), (k, R.prefix_next(k))]
    rs += [(ks[0], ks[len(ks) // 2]), (ks[len(ks) // 4], ks[-1]), (ks[len(ks) // 4], ks[-1])]  # overlapping, identical
    return rs


class Layout:
    """the table layout of a fixture case"""

    def __init__(self, t):
        self.id, self.pk_is_handle, self.pk_offset, self.cols = t["id"], t["pk_is_handle"], t["pk_offset"], t["columns"]
        self.indexes = {ix["id"]: ix for ix in t["indexes"]}
        self.col_types = [R.type_of(c) for c in self.cols]
        self.handle_type = self.col_types[self.pk_offset] if self.pk_is_handle else abi.I64
        self.pk_status = PK_UNSIGNED if self.handle_type == abi.U64 else PK_SIGNED

    # ---- the readers' schemas
    def table_types(self):
        return self.col_types + ([] if self.pk_is_handle else [abi.I64])

    def table_handle_idx(self):
        return self.pk_offset if self.pk_is_handle else len(self.cols)

    def index_types(self, ix):
        return [self.col_types[c] for c in self.indexes[ix]["columns"]] + [self.handle_type]

    def col_infos(self):
        """the table reader's rowcodec.ColInfos: the columns, then the extra handle column of a table without PK-is-handle"""
        out = []
        for i, c in enumerate(self.cols):
            tp = RC.TypeVarchar if c["type"] == "varchar" else RC.TypeLong
            out.append(RC.ColInfo(c["id"], tp, RC.UnsignedFlag if c.get("unsigned") else 0, self.pk_is_handle and i == self.pk_offset))
        if not self.pk_is_handle:
            out.append(RC.ColInfo(-1, RC.TypeLonglong, 0, True))
        return out

    def specs(self):
        """the same as the oracle's rowcodec column specs"""
        return [(c.ID, c.tsq_type(), abi.RC_HANDLE if c.IsPKHandle else 0, 0) for c in self.col_infos()]

    def table_row(self, row):
        return tuple(self._cell(i, v) for i, v in enumerate(row[1:])) + (() if self.pk_is_handle else (row[0],))

    def index_row(self, ix, row):
        return tuple(self._cell(c, row[1 + c]) for c in self.indexes[ix]["columns"]) + (row[0],)

    def _cell(self, i, v):
        return v.encode() if isinstance(v, str) else v

    # ---- the KV pairs of one row [handle, cell, ...]
    def kv(self, orc, row):
        h = int(row[0])
        stored = [i for i in range(len(self.cols)) if not (self.pk_is_handle and i == self.pk_offset)]
        vals, offs = orc.rowcodec_encode(Chunk([cell_column(self.col_types[i], [self._cell(i, row[1 + i])]) for i in stored]), [self.cols[i]["id"] for i in stored])
        out = [(R.record_key(self.id, h), bytes(vals[:offs[1]]))]
        for ix in self.indexes.values():
            cells = [self._cell(c, row[1 + c]) for c in ix["columns"]]
            in_key = 1 if not ix["unique"] or any(v is None for v in cells) else 0
            k, ko = orc.encode_index_keys(Chunk([cell_column(self.col_types[c], [v]) for c, v in zip(ix["columns"], cells)]), self.id, ix["id"],
                                          np.array([h], dtype=np.int64), np.array([in_key], dtype=np.uint8))
            out.append((bytes(k[:ko[1]]), b"0" if in_key else h.to_bytes(8, "big", signed=True)))
        return out


class Txn:
    """the steps of a case replayed into `buffers` (objects with Set / Delete: the dict model, a kv.MemBuffer) and into the sequential
    DirtyTable model"""

    def __init__(self, orc, layout, committed, buffers):
        self.orc, self.layout, self.buffers = orc, layout, list(buffers)
        self.committed = {int(r[0]): r for r in committed}
        self.live = dict(self.committed)
        self.dirty = R.DirtyTableRef()

    def insert(self, rows):
        for r in rows:
            for k, v in self.layout.kv(self.orc, r):
                for b in self.buffers:
                    b.Set(k, v)
            self.live[int(r[0])] = r
            self.dirty.AddRow(r[0])

    def delete(self, handles):
        for h in handles:
            for k, _ in self.layout.kv(self.orc, self.live.pop(int(h))):
                for b in self.buffers:
                    b.Delete(k)
            self.dirty.DeleteRow(h)


def predicate(types, triples):
    ops = {"eq": lambda a, b: a == b, "gt": lambda a, b: a > b, "ge": lambda a, b: a >= b}

    def pred(row):
        for col, op, const in triples:
            v = row[col]
            if op == "notnull":
                if v is None:
                    return False
            elif v is None or not ops[op](v, const.encode() if isinstance(const, str) else const):
                return False
        return True
    return pred if triples else None


def expressions(types, triples):
    out = []
    for col, op, const in triples:
        c = E.Column(col, types[col])
        if op == "notnull":
            out.append(E.ScalarFunction("not", E.ScalarFunction("isnull", c)))
        else:
            out.append(E.ScalarFunction(op, c, E.Constant(const, unsigned=types[col] == abi.U64)))
    return out


class Read:
    """one read step: everything both sides need"""

    def __init__(self, layout, txn, spec):
        self.kind, self.desc, self.spec = spec["reader"], bool(spec["desc"]), spec
        self.index = spec.get("index")
        L = layout
        committed = list(txn.committed.values())
        if self.kind == "index":
            self.types, self.used_index, self.handle_idx = L.index_types(self.index), list(range(len(L.indexes[self.index]["columns"]))), len(L.indexes[self.index]["columns"])
            p = R.index_prefix(L.id, self.index)
            self.ranges = [(p, R.prefix_next(p))]
            snap = [L.index_row(self.index, r) for r in committed]
        else:
            self.types, self.handle_idx = L.table_types(), L.table_handle_idx()
            self.used_index = [] if self.kind == "table" else list(L.indexes[self.index]["columns"])
            if self.kind == "table" and spec["ranges"] != "full":
                hs = spec["ranges"]["handle_points"]
                self.ranges = [(R.record_key(L.id, h), R.prefix_next(R.record_key(L.id, h))) for h in hs]
                committed = [r for r in committed if r[0] in hs]
            elif self.kind == "table":
                p = R.record_prefix(L.id)
                self.ranges = [(p, R.prefix_next(p))]
            else:
                p = R.index_prefix(L.id, self.index)
                self.ranges = [(p, R.prefix_next(p))]
            snap = [L.table_row(r) for r in committed]
        order = functools.cmp_to_key(UnionScanRef(self.types, [], [], [], self.used_index, self.handle_idx, self.desc).scan_cmp)
        self.pred = predicate(self.types, spec["conditions"])
        self.snapshot = sorted([r for r in snap if self.pred is None or self.pred(r)], key=order)  # (the child reader has the conditions too)
        self.conditions = expressions(self.types, spec["conditions"])
        self.expect = [tuple(v.encode() if isinstance(v, str) else v for v in r) for r in spec["expect"]]

    def project(self, rows):
        return [tuple(r[c] for c in self.spec["project"]) for r in rows]

    def model_rows(self, orc, layout, model):
        """the mem reader's rows through tests/memread_ref.py"""
        L = layout
        if self.kind == "table":
            return R.mem_table_reader(orc, model, L.specs(), self.ranges, self.desc, self.pred)
        if self.kind == "index":
            t = self.types
            return R.mem_index_reader(orc, model, t, L.pk_status, list(range(len(t))), self.ranges, self.desc, self.pred)
        return R.mem_index_lookup_reader(orc, model, L.index_types(self.index), L.pk_status, L.id, L.specs(), self.ranges, self.desc, self.pred)
