"""Plain Python restatement of the mem readers (executor/mem_reader.go) and of the dirty handles of a table, built on the dict model of
the transaction buffer (tests/membuf_ref.Model): iterTxnMemBuffer (:256-281) over memDbBuffer.Iter, the three readers' getMemRows
(:67-109, :188-213, :359-398) with the oracle's row and index decoders, a Python predicate and reverseDatumSlice, and the two handle
sets tsq_membuf_dirty reads out of the buffer — beside a second, sequential model of executor.DirtyTable (union_scan.go:56-74) fed
statement by statement, which is what the reference keeps.  The host build of tsq_memread_dp.h and the GPU are held to this file."""
import numpy as np

from tests import membuf_ref as MR
from tinysql_amd import _abi as abi

ROWKEY_LEN = 19
flip = lambda v: ((int(v) + (1 << 63)) & ((1 << 64) - 1)).to_bytes(8, "big")


def record_prefix(table_id):
    return b"t" + flip(table_id) + b"_r"


def index_prefix(table_id, index_id):
    return b"t" + flip(table_id) + b"_i" + flip(index_id)


def record_key(table_id, handle):
    return record_prefix(table_id) + flip(handle)


def prefix_next(key):
    b = bytearray(key)
    for i in range(len(b) - 1, -1, -1):
        b[i] = (b[i] + 1) & 0xFF
        if b[i] != 0:
            return bytes(b)
    return bytes(key) + b"\x00"


def entries(model):
    """[(op, key, value)] of the finished buffer in key order, lock-only keys included (the device keeps them; the reference's buffer
    does not)"""
    return model.mutations()["entries"]


def in_range(k, start, end):
    """start <= k < end under bytes.Compare; an empty start is the first key; an empty end is 'to the last key' (the pinned departure)"""
    return k >= start and (not end or k < end)


def iter_txn_mem_buffer(model, ranges):
    """-> dict(pairs=[(key, value)] range by range in the order given, range_counts, positions, skipped_dels)"""
    ents = entries(model)
    pairs, counts, positions, dels = [], [], 0, 0
    for start, end in ranges:
        c = 0
        for op, k, v in ents:
            if not in_range(k, start, end):
                continue
            positions += 1
            if op == MR.OP_DEL:  # len(iter.Value()) == 0
                dels += 1
            elif op == MR.OP_PUT:
                pairs.append((k, v))
                c += 1
        counts.append(c)
    return dict(pairs=pairs, range_counts=counts, positions=positions, skipped_dels=dels)


def scan(model, ranges, desc=False):
    """tsq_membuf_scan: iter_txn_mem_buffer with the WHOLE sequence reversed for desc"""
    got = iter_txn_mem_buffer(model, ranges)
    if desc:
        got["pairs"] = got["pairs"][::-1]
    return got


def scan_points(model, keys):
    """tsq_membuf_scan_points: key i yields its pair iff the buffer holds it as a PUT; positions counts the keys the device buffer holds"""
    held = {k: (op, v) for op, k, v in entries(model)}
    pairs = [(k, held[k][1]) for k in keys if k in held and held[k][0] == MR.OP_PUT]
    return dict(pairs=pairs, range_counts=[int(k in held and held[k][0] == MR.OP_PUT) for k in keys], positions=sum(k in held for k in keys),
                skipped_dels=sum(k in held and held[k][0] == MR.OP_DEL for k in keys))


class InvalidKey(Exception):
    pass


def dirty_sets(model, table_id):
    """tsq_membuf_dirty: (added, deleted) handle lists, ascending — a PUT record key of the table is added, a DEL one deleted"""
    lo, hi = record_prefix(table_id), record_prefix(table_id)[:-1] + b"s"
    added, deleted = [], []
    for op, k, _ in entries(model):
        if not (lo <= k < hi):
            continue
        if len(k) != ROWKEY_LEN:
            raise InvalidKey(k)
        h = int.from_bytes(k[11:], "big") - (1 << 63)
        if op == MR.OP_PUT:
            added.append(h)
        elif op == MR.OP_DEL:
            deleted.append(h)
    return sorted(added), sorted(deleted)


class DirtyTableRef:
    """executor.DirtyTable fed statement by statement: AddRow leaves the deleted set alone, DeleteRow takes the handle out of the added set"""

    def __init__(self):
        self.addedRows, self.deletedRows = set(), set()

    def AddRow(self, h):
        self.addedRows.add(int(h))

    def DeleteRow(self, h):
        self.addedRows.discard(int(h))
        self.deletedRows.add(int(h))


# ---------------------------------------------------------------------------------------------------- the three readers
def _pack(cells):
    offs = np.zeros(len(cells) + 1, dtype=np.int64)
    if cells:
        offs[1:] = np.cumsum([len(c) for c in cells])
    return np.frombuffer(b"".join(cells), dtype=np.uint8).copy(), offs


def decode_table_rows(orc, pairs, specs):
    """[(record key, stored row)] -> rows (tuples, None = NULL); specs = the oracle's rowcodec column specs of the reader's ColInfos"""
    if not pairs:
        return []
    handles = [orc.decode_row_key(k) for k, _ in pairs]  # raises ValueError("invalid key")
    vals, offs = _pack([v for _, v in pairs])
    st, chk = orc.rowcodec_decode_chunk(vals, offs, np.array(handles, dtype=np.int64), specs)
    assert st == 0, st
    return chk.rows()


def decode_index_rows(orc, pairs, types, pk_status):
    """[(index key, value)] -> rows of (index columns..., handle); types: the index columns' and, last, the handle's"""
    if not pairs:
        return []
    keys, ko = _pack([k for k, _ in pairs])
    vals, vo = _pack([v for _, v in pairs])
    st, chk = orc.decode_index_kv(keys.tobytes(), ko, vals.tobytes(), vo, len(types) - 1, types, pk_status)
    assert st == 0, st
    return chk.rows()


def _finish(rows, pred, desc):
    rows = [r for r in rows if pred is None or pred(r)]
    return rows[::-1] if desc else rows


def mem_table_reader(orc, model, specs, ranges, desc=False, pred=None):
    return _finish(decode_table_rows(orc, iter_txn_mem_buffer(model, ranges)["pairs"], specs), pred, desc)


def mem_index_reader(orc, model, types, pk_status, output_offset, ranges, desc=False, pred=None):
    rows = [tuple(r[o] for o in output_offset) for r in decode_index_rows(orc, iter_txn_mem_buffer(model, ranges)["pairs"], types, pk_status)]
    return _finish(rows, pred, desc)


def signed(h):
    h = int(h) & ((1 << 64) - 1)
    return h - (1 << 64) if h >> 63 else h


def mem_index_lookup_reader(orc, model, types, pk_status, table_id, specs, ranges, desc=False, pred=None):
    """the handles of the index scan (reversed for desc), one point range per handle in that order, the table decode, the predicate; the
    table side is not reversed a second time"""
    handles = [signed(r[0]) for r in mem_index_reader(orc, model, types, pk_status, [len(types) - 1], ranges, desc)]
    pairs = scan_points(model, [record_key(table_id, h) for h in handles])["pairs"]
    return _finish(decode_table_rows(orc, pairs, specs), pred, False)


def type_of(col):
    """a fixture column -> the chunk column type"""
    if col["type"] == "varchar":
        return abi.BYTES
    return abi.U64 if col.get("unsigned") else abi.I64
