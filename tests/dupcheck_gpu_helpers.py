"""Drives tsq_dupcheck_* / tsq_rows_equal on the device for a statement given as Python rows (the shapes of tests/dupcheck_ref.py): the
store's streams are built from the model's keys, the statement's keys by the product's own encoders (tablecodec.GenIndexKeys on the
device chunk), and everything that comes back is returned in host form, to be compared with the model."""
import numpy as np

from tests import dupcheck_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import dupcheck as D
from tinysql_amd import tablecodec
from tinysql_amd.gpu_pipeline import DeviceChunk

GUARD = 64  # bytes of pattern on each side of an output array
PATTERN = 0x5A


class Guarded:
    """a device output array between two guard zones"""

    def __init__(self, ctx, nbytes):
        self.ctx, self.nbytes = ctx, nbytes
        self.base = ctx.alloc(nbytes + 2 * GUARD + 64)
        ctx.memset(self.base, PATTERN, nbytes + 2 * GUARD)
        self.p = self.base + GUARD

    def read(self, dtype, count):
        raw = np.zeros(self.nbytes + 2 * GUARD, np.uint8)
        self.ctx.d2h(raw, self.base)
        assert (raw[:GUARD] == PATTERN).all() and (raw[GUARD + self.nbytes:] == PATTERN).all(), "an output array was written outside its bounds"
        return raw[GUARD:GUARD + self.nbytes].view(dtype)[:count].copy()

    def free(self):
        self.ctx.free(self.base)


class Statement:
    """the store and the statement of one case in HBM"""

    def __init__(self, ctx, shape, stored, rows):
        self.ctx, self.shape, self.rows, self.n = ctx, shape, [tuple(r) for r in rows], len(rows)
        self.stored = sorted(stored)
        self.keep = []
        self.table_handles = np.array([h for h, _ in self.stored], dtype=np.int64)
        self.d_table = self.up(self.table_handles)
        self.streams = []
        if shape.pk_col is not None:
            self.streams.append(D.HandleStream(self.d_table.p, len(self.stored)))
        for i in range(len(shape.uniques)):
            self.streams.append(self.index_stream(i))
        self.chunk = DeviceChunk.from_host(ctx, R.chunk_of(shape.col_types, self.rows))
        self.old = DeviceChunk.from_host(ctx, R.chunk_of(shape.col_types, [r for _, r in self.stored]))
        self.d_zero = self.up(np.zeros(max(self.n, 1), np.int64))
        self.row_handles = self.chunk.columns[shape.pk_col].data if shape.pk_col is not None else self.d_zero.p
        self.kvs = []
        for u in shape.uniques if self.n else ():
            sub = DeviceChunk([self.chunk.columns[c] for c, _ in u], self.n)
            self.kvs.append(tablecodec.GenIndexKeys(ctx, shape.table_id, len(self.kvs) + 1, True, sub, self.row_handles,
                                                    prefix_len=[-1 if p is None else p for _, p in u], prefix_utf8=[False] * len(u)))

    def up(self, host):
        a = D.DevArray(self.ctx, host)
        self.keep.append(a)
        return a

    def index_stream(self, i, float_key=False):
        ks, ds = R.index_keys(self.shape, i, [r for _, r in self.stored])
        ent = sorted((k, h) for k, d, (h, _) in zip(ks, ds, self.stored) if d)
        offs = np.zeros(len(ent) + 1, np.int64)
        np.cumsum([len(k) for k, _ in ent], out=offs[1:])
        raw = np.frombuffer(b"".join(k for k, _ in ent) + b"\0", np.uint8)
        return D.IndexStream(self.up(raw).p, self.up(offs).p, int(offs[-1]), self.up(np.array([h for _, h in ent], dtype=np.int64)).p, len(ent), float_key)

    def checker(self, mode, splits=None):
        """a DupChecker with the statement's keys pushed; splits: rows per push (None: one push)"""
        with_table = self.shape.pk_col is None
        chk = D.DupChecker(self.ctx, self.streams, mode, self.d_table.p if with_table else None, len(self.stored) if with_table else 0)
        try:
            self.push_into(chk, splits)
        except Exception:
            chk.close()
            raise
        return chk

    def push_into(self, chk, splits=None):
        step = splits or max(self.n, 1)
        for lo in range(0, max(self.n, 1), step):
            m = min(step, self.n - lo)
            keys = []
            if self.shape.pk_col is not None:
                keys.append(self.row_handles + 8 * lo)
            for kv in self.kvs:
                keys.append((kv.keys, kv.key_offsets + 8 * lo, kv.nbytes, kv.distinct + lo))
            keys += [(None, None, 0, None)] * (len(self.streams) - len(keys))  # (an empty statement: nothing was encoded)
            chk.push(keys, m)

    def insert(self, splits=None):
        """-> None or the KeyExistsError"""
        chk = self.checker(abi.DUP_INSERT, splits)
        try:
            return chk.match_insert()
        finally:
            chk.close()

    def replace(self, rowid_base=0, splits=None, cap_removed=None):
        """-> dict in the model's terms (+ cand: the candidate of every row as the form names it)"""
        n, ctx = self.n, self.ctx
        chk = self.checker(abi.DUP_REPLACE, splits)
        outs = []

        def out(nbytes):
            g = Guarded(ctx, nbytes)
            outs.append(g)
            return g
        try:
            c_row, c_handle, c_ord = out(8 * n), out(8 * n), out(8 * n)
            nb, ns = chk.match_replace(c_row.p, c_handle.p, c_ord.p)
            cand_row, cand_handle, cand_ord = c_row.read(np.int64, n), c_handle.read(np.int64, n), c_ord.read(np.int64, n)
            assert nb == int((cand_row >= 0).sum()) and ns == int(((cand_row < 0) & (cand_ord >= 0)).sum())
            assert (self.table_handles[cand_ord[cand_ord >= 0]] == cand_handle[cand_ord >= 0]).all()
            # EqualDatums against the candidates: once against the statement's own rows, once against the stored rows
            f1, f2 = out(n), out(n)
            cols = [c.col(n) for c in self.chunk.columns]
            D.rows_equal(ctx, cols, None, cols, c_row.p, n, f1.p)
            D.rows_equal(ctx, cols, None, [c.col(len(self.stored)) for c in self.old.columns], c_ord.p, n, f2.p)
            eq = f1.read(np.uint8, n) | f2.read(np.uint8, n)
            d_eq = self.up(eq if n else np.zeros(1, np.uint8))
            cap = min(n * len(self.streams), len(self.stored)) if cap_removed is None else cap_removed
            added, put, handles, r_h, r_o = out(n), out(n), out(8 * n), out(8 * cap), out(8 * cap)
            res = chk.resolve(d_eq.p, rowid_base, added.p, put.p, handles.p, r_h.p, r_o.p, cap)
            k = res.n_removed_store
            removed_handles, removed_ords = r_h.read(np.int64, k), r_o.read(np.int64, k)
            assert (self.table_handles[removed_ords] == removed_handles).all()
            a, p, hs = added.read(np.uint8, n).astype(bool), put.read(np.uint8, n).astype(bool), handles.read(np.int64, n)
            assert res.n_added == int(a.sum()) and res.n_put == int(p.sum()) and res.n_removed_batch == res.n_added - res.n_put
            assert (hs[~a] == 0).all()
            pk = self.shape.pk_col
            row_handles = [None if not a[r] else (self.rows[r][pk] if pk is not None else int(hs[r])) for r in range(n)]
            table = {h: r for h, r in self.stored if h not in set(removed_handles.tolist())}
            for r in range(n):
                if p[r]:
                    table[row_handles[r]] = self.rows[r]
            cand = [("b", int(cand_row[r])) if cand_row[r] >= 0 else (("s", int(cand_handle[r])) if cand_ord[r] >= 0 else None) for r in range(n)]
            return dict(cand=cand, equal=eq.astype(bool).tolist(), added=a.tolist(), put=p.tolist(), handles=row_handles, removed_store=removed_handles.tolist(),
                        n_removed_batch=res.n_removed_batch, affected=res.affected, rowid_base=res.rowid_base if pk is None else rowid_base, table=table,
                        stats=chk.stats())
        finally:
            chk.close()
            for g in outs:
                g.free()

    def free(self):
        for kv in self.kvs:
            kv.free()
        self.chunk.free()
        self.old.free()
        for a in self.keep:
            a.free()


def check_replace(ctx, shape, stored, rows, rowid_base=0, splits=None):
    """runs the statement on the device and holds every output to the sequential model (and the candidates to the form)"""
    from tests import dupcheck_form as F
    st = Statement(ctx, shape, stored, rows)
    try:
        got = st.replace(rowid_base, splits)
    finally:
        st.free()
    store = R.Store(shape, stored)
    want = R.replace_stmt(shape, store, [tuple(r) for r in rows], rowid_base)
    form = F.parallel_replace(shape, sorted(stored), [tuple(r) for r in rows], rowid_base)
    assert got["cand"] == form["cand"] and got["equal"] == form["equal"]
    for k in ("added", "put", "handles", "removed_store", "n_removed_batch", "affected", "rowid_base"):
        assert got[k] == want[k], k
    assert repr(sorted(got["table"].items())) == repr(sorted(store.table().items()))
    return got, want


def check_insert(ctx, shape, stored, rows, rowid_base=0, splits=None):
    st = Statement(ctx, shape, stored, rows)
    try:
        got = st.insert(splits)
    finally:
        st.free()
    try:
        R.insert_stmt(shape, R.Store(shape, stored), [tuple(r) for r in rows], rowid_base)
        want = None
    except R.KeyExists as e:
        want = e
    if want is None:
        assert got is None, got
        return None
    assert got is not None and (got.row, got.stream) == (want.row, want.stream)
    if got.from_store:
        assert got.dup_handle == want.dup_handle and got.dup_row == -1
    else:  # the entry of the FIRST row of the key's group; without a PK handle that row took rowid_base + its position + 1
        pk = shape.pk_col
        assert 0 <= got.dup_row < got.row
        assert (rows[got.dup_row][pk] if pk is not None else rowid_base + got.dup_row + 1) == want.dup_handle
    return got
