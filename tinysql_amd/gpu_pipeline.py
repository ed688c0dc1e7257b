"""Device-resident volcano operators: the same Open / Next / Close contract as `executor.py`
(executor/executor.go:146-162), but the chunks handed from child to parent stay in HBM.

SURVEY.md §8(f) rank 1: when parent and child are both GPU operators the D2H -> H2D hop of a 1024-row
host chunk is replaced by a pointer hand-off; `tidb_max_chunk_size` has no upper bound
(sessionctx/variable/varsutil.go:251), so a "chunk" here is millions of rows.  Everything below is host
plumbing around the C-ABI (`include/tsq.h`); all compute runs in libtsq:
  GpuSelectionExec   = tsq_filter_eval (device flags) + tsq_chunk_compact  (executor.go:346-438, column.go:504-552)
  GpuProjectionExec  = tsq_expr_eval per output column                     (projection.go:54-434, evaluator.go:121-133)
  GpuSelectProjectExec = tsq_project_* : the two above as ONE operator (opt-in; filter once, all outputs in one kernel)
  GpuHashJoinExec    = tsq_join_* with TSQ_COL_DEVICE columns              (join.go:31-146)
  GpuHashAggExec     = tsq_agg_* with TSQ_COL_DEVICE columns               (aggregate.go:134-588)
  GpuSortExec        = tsq_sort_* (ORDER BY / TopN) with TSQ_COL_DEVICE columns (sort.go:27-318)
  GpuReplaceSelectExec = GpuInsertSelectExec's casts and ids + tsq_chunk_append + tsq_dupcheck_* (REPLACE mode) + tsq_rows_equal + the encoders (replace.go:53-196)
  GpuUnionScanExec   = tsq_unionscan_* with TSQ_COL_DEVICE columns             (union_scan.go:89-300)
  GpuIndexLookUpExecutor = coprocessor.tableLookupExec per task (tsq_lookup_task + tsq_rows_gather + tsq_rowcodec_decode) (distsql.go:237-637)
  GpuInsertSelectExec = tsq_cast_run + tsq_autoid_fill + tsq_rowkeys_encode + tsq_rowcodec_encode + tsq_indexkeys_encode (insert_common.go:340-401)
                        (+ with store=: tsq_dupcheck_* in INSERT mode, the duplicate-key check of tables.AddRecord, tables.go:528-581)
A chunk returned by Next is valid until the next call of Next on the same operator (the Go operators
recycle their chunks the same way, join.go:62-78).
"""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib
from .chunk import Chunk, Column, StrColumn, np_dtype
from .expression import Column as Column_
from .expression import ETReal, ETString, CompiledExpr, Unsupported, compile_list


def _es(tp):
    return 4 if tp == abi.F32 else 8


class DeviceColumn:
    """one column in HBM: data + optional null bitmap (bit 1 = NOT NULL, util/chunk/column.go:89-92); a var-len (abi.BYTES)
    column also has offsets[cap + 1] and its data buffer holds `cap_bytes` bytes (column.go:28-34)."""

    def __init__(self, ctx, tp, cap_rows, with_bitmap=True, data=None, bitmap=None, offsets=None, cap_bytes=0):
        self.ctx, self.tp, self.cap = ctx, tp, cap_rows
        self.var = tp == abi.BYTES
        self.cap_bytes = cap_bytes
        self.owned = data is None
        if self.owned:
            self.data = ctx.alloc((max(cap_bytes, 1) if self.var else max(cap_rows, 1) * _es(tp)) + 64)
            self.bitmap = ctx.alloc((cap_rows + 7) // 8 + 64) if with_bitmap else None
            self.offsets = ctx.alloc((cap_rows + 1) * 8 + 64) if self.var else None
        else:
            self.data, self.bitmap, self.offsets = data, bitmap, offsets

    def col(self, nrows):
        c = abi.Col()
        c.data, c.null_bitmap, c.length = self.data, self.bitmap, nrows
        c.offsets = self.offsets if self.var else None
        c.elem_size, c.type, c.flags = (-1 if self.var else _es(self.tp)), self.tp, abi.COL_DEVICE
        return c

    def view(self, lo):
        """rows [lo, ...) — lo must be a multiple of 8 so that the bitmap stays byte aligned.  A var-len view keeps the data
        base: the offsets index it (the rows' offsets need not start at 0, tsq_colset_slice)."""
        assert lo % 8 == 0
        if self.var:
            return DeviceColumn(self.ctx, self.tp, self.cap - lo, data=self.data, offsets=self.offsets + 8 * lo, cap_bytes=self.cap_bytes,
                                bitmap=None if self.bitmap is None else self.bitmap + lo // 8)
        return DeviceColumn(self.ctx, self.tp, self.cap - lo, data=self.data + lo * _es(self.tp),
                            bitmap=None if self.bitmap is None else self.bitmap + lo // 8)

    def nbytes(self, nrows):
        """data bytes spanned by the first nrows cells of a var-len column (one 16-byte read-back)"""
        if not self.var or nrows == 0:
            return 0
        o = np.zeros(1, np.int64)
        e = np.zeros(1, np.int64)
        self.ctx.d2h(o, self.offsets)
        self.ctx.d2h(e, self.offsets + 8 * nrows)
        return int(e[0] - o[0])

    def ensure_bytes(self, nbytes):
        """grow the data buffer of an owned var-len column (contents are not kept: called before a pull fills it)"""
        if self.var and nbytes > self.cap_bytes:
            assert self.owned
            self.ctx.free(self.data)
            self.cap_bytes = int(nbytes * 1.25) + 64
            self.data = self.ctx.alloc(self.cap_bytes + 64)

    def to_host_pinned(self, nrows):
        """fixed-width column -> (data array, bitmap bytes or None) in PINNED host memory (ctx.host_array): one DMA each, no
        pageable bounce, no unpacking — the form a host operator consumes (util/chunk/column.go:28-34 keeps the bitmap packed too)"""
        assert not self.var
        data = self.ctx.host_array(max(nrows, 1), np_dtype(self.tp))
        self.ctx.d2h(data, self.data)
        bm = None
        if self.bitmap is not None:
            bm = self.ctx.host_array((nrows + 7) // 8 + 1, np.uint8)
            self.ctx.d2h(bm, self.bitmap)
        return data, bm

    def to_host(self, nrows):
        nn = None
        if self.bitmap is not None:
            bm = np.zeros((nrows + 7) // 8 + 1, np.uint8)
            self.ctx.d2h(bm, self.bitmap)
            nn = np.unpackbits(bm, bitorder="little")[:nrows].astype(bool)
        if self.var:
            offs = np.zeros(nrows + 1, np.int64)
            self.ctx.d2h(offs, self.offsets)
            lo, hi = int(offs[0]), int(offs[nrows])
            raw = np.zeros(max(hi - lo, 1), np.uint8)
            if hi > lo:
                self.ctx.d2h(raw, self.data + lo)
            return StrColumn([bytes(raw[offs[r] - lo:offs[r + 1] - lo]) if (nn is None or nn[r]) else None for r in range(nrows)])
        arr = np.zeros(max(nrows, 1), dtype=np_dtype(self.tp))
        self.ctx.d2h(arr, self.data)
        return Column(self.tp, arr[:nrows].copy(), nn)

    def free(self):
        if self.owned:
            self.ctx.free(self.data)
            if self.bitmap is not None:
                self.ctx.free(self.bitmap)
            if self.offsets is not None:
                self.ctx.free(self.offsets)
        self.data = self.bitmap = self.offsets = None


class DeviceChunk:
    def __init__(self, columns, nrows, sel=None):
        # sel: device pointer to one byte per row, 0 = the row was filtered out (Chunk.sel of the reference is a selection VECTOR,
        # util/chunk/chunk.go:31-46; a flag per row is its device form).  Only operators that say so accept a chunk with sel.
        self.columns, self.nrows, self.sel = list(columns), nrows, sel

    def NumRows(self):
        return self.nrows

    def types(self):
        return [c.tp for c in self.columns]

    def cols(self):
        return (abi.Col * len(self.columns))(*[c.col(self.nrows) for c in self.columns])

    def to_host(self):
        return Chunk([c.to_host(self.nrows) for c in self.columns])

    def free(self):
        for c in self.columns:
            c.free()

    def append(self, ctx, src):
        """device-side Chunk.Append (tsq_chunk_append): the rows of the device chunk `src` behind this chunk's rows.  This chunk owns its
        columns (with null bitmaps); a column that has no room grows by half, its rows moved by the same call."""
        n = src.NumRows()
        if n == 0:
            return
        for i, (d, s) in enumerate(zip(self.columns, src.columns)):
            assert d.owned and d.bitmap is not None and d.tp == s.tp
            rows, nb = self.nrows + n, d.nbytes(self.nrows) + s.nbytes(n)
            if rows > d.cap or nb > d.cap_bytes:
                g = DeviceColumn(ctx, d.tp, max(rows, d.cap + d.cap // 2), cap_bytes=max(nb, d.cap_bytes + d.cap_bytes // 2) if d.var else 0)
                try:
                    _chunk_append(ctx, [g], 0, [d], self.nrows)
                except Exception:
                    g.free()
                    raise
                d.free()
                self.columns[i] = g
        _chunk_append(ctx, self.columns, self.nrows, src.columns, n)
        self.nrows += n

    @staticmethod
    def from_host(ctx, chunk):
        """a host chunk copied to HBM; a column without a NOT-NULL array (a NOT NULL column) gets no null bitmap"""
        cols = []
        for c in chunk.columns:
            has_nulls = c.notnull is not None
            if c.tp == abi.BYTES:
                nb = int(c.offsets[-1]) if len(c.offsets) else 0
                d = DeviceColumn(ctx, c.tp, len(c), with_bitmap=has_nulls, cap_bytes=nb)
                if nb:
                    ctx.h2d(d.data, np.ascontiguousarray(c.data[:nb]))
                ctx.h2d(d.offsets, np.ascontiguousarray(c.offsets))
            else:
                d = DeviceColumn(ctx, c.tp, len(c), with_bitmap=has_nulls)
                ctx.h2d(d.data, np.ascontiguousarray(c.data))
            if len(c) and has_nulls:
                ctx.h2d(d.bitmap, np.packbits(c.notnull, bitorder="little"))
            cols.append(d)
        return DeviceChunk(cols, chunk.NumRows())


def _chunk_append(ctx, dst, dst_rows, src, n):
    nc = len(dst)
    dc = (abi.Col * nc)(*[c.col(c.cap) for c in dst])
    sc = (abi.Col * nc)(*[c.col(n) for c in src])
    caps = (C.c_int64 * nc)(*[c.cap_bytes for c in dst])
    _lib.check(ctx.lib.tsq_chunk_append(ctx.h, dc, dst_rows, caps, sc, nc, n), ctx.h)


class GpuExecutor:
    def __init__(self, ctx, types, children=()):
        self.ctx, self.lib, self.types, self.children = ctx, ctx.lib, list(types), list(children)

    def Schema(self):
        return self.types

    def Open(self):
        for c in self.children:
            c.Open()

    def Close(self):
        for c in self.children:
            c.Close()

    def _buffers(self, cap_rows, var_bytes=None):
        """output columns for up to cap_rows rows; var_bytes[i]: data bytes of var-len column i (grown later by ensure_bytes)"""
        return [DeviceColumn(self.ctx, t, cap_rows, cap_bytes=(var_bytes[i] if var_bytes else 0) if t == abi.BYTES else 0) for i, t in enumerate(self.types)]

    def _size_varlen(self, peek, handle, out, cap_rows):
        """before a pull: ask how many data bytes the var-len output columns of the next pull need and grow their buffers"""
        if abi.BYTES not in self.types:
            return
        vb, nr = (C.c_int64 * len(self.types))(), C.c_int64(0)
        _lib.check(peek(handle, cap_rows, C.byref(nr), vb, len(self.types)), handle)
        for c, b in zip(out, vb):
            c.ensure_bytes(b)


EOS = DeviceChunk([], 0)


def drain_device(exe):
    """Open / Next* / Close; returns host Chunks (the root of a plan copies its result out like writeChunks does)."""
    exe.Open()
    out = []
    try:
        while True:
            chk = exe.Next()
            if chk.NumRows() == 0:
                break
            out.append(chk.to_host())
    finally:
        exe.Close()
    return out


class DeviceTableScan(GpuExecutor):
    """a table that already lives in HBM (what a GPU-side TableReader / cop-response decoder would produce), handed out in
    batches of `batch_rows` rows as pointer views."""

    def __init__(self, ctx, table, batch_rows=1 << 24):
        super().__init__(ctx, table.types())
        self.table, self.batch, self.pos = table, (batch_rows + 7) & ~7, 0

    def Open(self):
        self.pos = 0

    def Next(self):
        n = self.table.nrows
        if self.pos >= n:
            return EOS
        hi = min(n, self.pos + self.batch)
        out = DeviceChunk([c.view(self.pos) for c in self.table.columns], hi - self.pos)
        self.pos = hi
        return out


class GpuSelectionExec(GpuExecutor):
    def __init__(self, ctx, child, filters, jit=None, compact=True, str_ctx=0):
        """compact=False: the chunk is handed on UNCOMPACTED with its selection flags (DeviceChunk.sel) — for a parent that takes them
        (GpuHashJoinExec's probe side: tsq_join_probe_push(selected)): the filtered rows are never copied.  str_ctx: the statement's
        string-to-int flags (abi.STRCTX_*) for string-valued conjuncts; their warnings add up in self.truncated_warnings /
        self.overflow_warnings (kept after Close)."""
        super().__init__(ctx, child.Schema(), (child,))
        self.child, self.filters, self.jit, self.compact, self.str_ctx = child, list(filters), jit, compact, str_ctx
        self.expr, self.out, self.flags, self.cap = None, None, None, 0
        self.truncated_warnings = self.overflow_warnings = 0

    def Open(self):
        super().Open()
        self.expr = CompiledExpr(self.ctx, self.filters, jit=self.jit, str_ctx=self.str_ctx)
        self.truncated_warnings = self.overflow_warnings = 0

    def Next(self):
        while True:
            chk = self.child.Next()
            n = chk.NumRows()
            if n == 0:
                return EOS
            if n > self.cap:
                self._release()
                self.cap = n
                self.out = self._buffers(n) if self.compact else []
                self.flags = self.ctx.alloc(n + 64)
            w = C.c_int64(0)
            st = self.lib.tsq_filter_eval(self.expr.h, chk.cols(), len(chk.columns), n, None, self.flags, None, C.byref(w))
            self.expr.warnings += w.value
            t, o = C.c_int64(0), C.c_int64(0)
            self.lib.tsq_expr_str_warnings(self.expr.h, C.byref(t), C.byref(o))
            self.truncated_warnings += t.value
            self.overflow_warnings += o.value
            _lib.check(st, self.expr.h)
            if not self.compact:
                return DeviceChunk(chk.columns, n, sel=self.flags)
            for src, dst in zip(chk.columns, self.out):  # a selection never grows a var-len column
                dst.ensure_bytes(src.nbytes(n))
            oc = (abi.Col * len(self.out))(*[c.col(n) for c in self.out])
            m = C.c_int64(0)
            _lib.check(self.lib.tsq_chunk_compact(self.ctx.h, chk.cols(), len(chk.columns), n, self.flags, oc, C.byref(m)), self.ctx.h)
            if m.value:
                return DeviceChunk(self.out, m.value)

    def _release(self):
        if self.out:
            for c in self.out:
                c.free()
        if self.flags:
            self.ctx.free(self.flags)
        self.out, self.flags, self.cap = None, None, 0

    def Close(self):
        self._release()
        if self.expr:
            self.expr.close()
            self.expr = None
        super().Close()


class GpuProjectionExec(GpuExecutor):
    def __init__(self, ctx, child, exprs, jit=None):
        # a string-valued expression has no fixed-width output column here: the planner must learn that when it BUILDS the plan
        # (Unsupported = keep the Go ProjectionExec), not from a failing Next
        for e in exprs:
            if e.eval_type == ETString:
                raise Unsupported("GpuProjectionExec: a string-valued projection expression keeps the Go operator (VecEvalString exists on chunk level only)")
        types = [abi.F64 if e.eval_type == ETReal else (abi.U64 if e.unsigned else abi.I64) for e in exprs]
        super().__init__(ctx, types, (child,))
        self.child, self.exprs, self.jit = child, list(exprs), jit
        self.compiled, self.out, self.cap = [], None, 0

    def Open(self):
        super().Open()
        # a bare 8-byte column needs no kernel: the child's column is handed on (the reference copies it, projection.go:54-62
        # -> Column.CopyConstruct; a device pointer that stays valid until the child's next Next is equivalent here)
        self.passthru = [e.index if isinstance(e, Column_) and e.tp != abi.F32 else None for e in self.exprs]
        self.compiled = [None if p is not None else CompiledExpr(self.ctx, [e], jit=self.jit) for p, e in zip(self.passthru, self.exprs)]

    def Next(self):
        chk = self.child.Next()
        n = chk.NumRows()
        if n == 0:
            return EOS
        if n > self.cap:
            self._release()
            self.cap = n
            self.out = [None if p is not None else DeviceColumn(self.ctx, t, n) for p, t in zip(self.passthru, self.types)]
        cols = []
        for p, ce, dst in zip(self.passthru, self.compiled, self.out):
            if p is not None:
                cols.append(chk.columns[p])
                continue
            oc = dst.col(n)
            oc.type = abi.F64 if dst.tp == abi.F64 else abi.I64
            w = C.c_int64(0)
            _lib.check(self.lib.tsq_expr_eval(ce.h, chk.cols(), len(chk.columns), n, None, C.byref(oc), C.byref(w)), ce.h)
            ce.warnings += w.value
            cols.append(dst)
        return DeviceChunk(cols, n)

    def _release(self):
        if self.out:
            for c in self.out:
                if c is not None:
                    c.free()
        self.out, self.cap = None, 0

    def Close(self):
        self._release()
        for ce in self.compiled:
            if ce is not None:
                ce.close()
        self.compiled = []
        super().Close()


class GpuSelectProjectExec(GpuExecutor):
    """SELECT exprs FROM child WHERE filters as one operator (tsq_project_*, ABI 10): ProjectionExec over SelectionExec, whose
    EvaluatorSuite.Run evaluates the whole SELECT list per chunk on the rows the selection kept (evaluator.go:46-63, executor.go:393-438).
    The filter runs once, one kernel evaluates every output for the selected rows (each input cell is loaded once per row) and only
    the outputs are written, dense and in input order; filters may be empty (a pure projection).  The chunk Next returns lives in
    buffers of the handle (borrowed): valid until the next Next / Close.  Division-by-zero warnings add up in self.warnings, the
    string conjuncts' in self.truncated_warnings / self.overflow_warnings, as in GpuSelectionExec."""

    def __init__(self, ctx, child, filters, exprs, jit=None, str_ctx=0):
        exprs, filters = list(exprs), list(filters)
        if not 1 <= len(exprs) <= 16 or len(filters) > 16:
            raise Unsupported("GpuSelectProjectExec: 1..16 output expressions and at most 16 conjuncts")
        types = [abi.BYTES if e.eval_type == ETString else (abi.F64 if e.eval_type == ETReal else (abi.U64 if e.unsigned else abi.I64)) for e in exprs]
        super().__init__(ctx, types, (child,))
        self.child, self.filters, self.exprs, self.jit, self.str_ctx = child, filters, exprs, jit, str_ctx
        self.fprogs = compile_list(filters, str_ctx)  # (raises Unsupported for what the interpreter cannot hold)
        self.oprogs = compile_list(exprs, str_ctx)
        self.h = None
        self.warnings = self.truncated_warnings = self.overflow_warnings = 0
        # what the library refuses is refused HERE, when the plan is built, not by a failing Next; the handle is kept for Open
        try:
            self._create()
        except _lib.TsqError as ex:
            raise Unsupported("GpuSelectProjectExec: %s" % ex)

    def _create(self):
        h = C.c_void_p()
        _lib.check(self.lib.tsq_project_create(self.ctx.h, self.fprogs if self.filters else None, len(self.filters), self.oprogs, len(self.exprs),
                                               C.byref(h)), self.ctx.h)
        self.h = h
        if self.jit is not None:
            _lib.check(self.lib.tsq_project_set_jit(h, self.jit), h)

    def _destroy(self):
        if self.h:
            self.lib.tsq_project_destroy(self.h)
            self.h = None

    def Open(self):
        super().Open()
        if not self.h:  # (a second Open after Close)
            self._create()
        self.warnings = self.truncated_warnings = self.overflow_warnings = 0

    def Next(self):
        while True:
            chk = self.child.Next()
            n = chk.NumRows()
            if n == 0:
                return EOS
            oc = (abi.Col * len(self.exprs))()
            m, w = C.c_int64(0), C.c_int64(0)
            st = self.lib.tsq_project_run(self.h, chk.cols(), len(chk.columns), n, oc, len(self.exprs), C.byref(m), C.byref(w))
            self.warnings += w.value
            t, o = C.c_int64(0), C.c_int64(0)
            self.lib.tsq_project_str_warnings(self.h, C.byref(t), C.byref(o))
            self.truncated_warnings += t.value
            self.overflow_warnings += o.value
            _lib.check(st, self.h)
            if m.value:
                cols = [DeviceColumn(self.ctx, c.type, m.value, data=c.data, bitmap=c.null_bitmap, offsets=c.offsets) for c in oc]
                return DeviceChunk(cols, m.value)

    def stats(self):
        """(launches of the evaluate-and-scatter kernel, those served by the specialised form, device ms of the most recent one)"""
        a, b, ms = C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_project_stats(self.h, C.byref(a), C.byref(b), C.byref(ms)), self.h)
        return a.value, b.value, ms.value

    def Close(self):
        self._destroy()
        super().Close()


class GpuHashJoinExec(GpuExecutor):
    def __init__(self, ctx, left, right, left_keys, right_keys, join_type=abi.JOIN_INNER, inner_child_idx=1, pull_rows=1 << 24, used=None):
        """used: the output columns (indices into left's + right's columns) the parent reads — the planner's column pruning
        (tsq_join_set_used_columns); the others are not materialised and come out as columns without data."""
        super().__init__(ctx, left.Schema() + right.Schema(), (left, right))
        self.used = None if used is None else sorted(set(used))
        self.build_is_right = inner_child_idx == 1
        self.build = right if self.build_is_right else left
        self.probe = left if self.build_is_right else right
        bkeys = right_keys if self.build_is_right else left_keys
        pkeys = left_keys if self.build_is_right else right_keys
        cfg = abi.JoinCfg()
        cfg.join_type, cfg.build_is_right, cfg.n_keys = join_type, 1 if self.build_is_right else 0, len(bkeys)
        for i, (b, p) in enumerate(zip(bkeys, pkeys)):
            cfg.build_key_idx[i], cfg.probe_key_idx[i] = b, p
        cfg.n_build_cols, cfg.n_probe_cols = len(self.build.Schema()), len(self.probe.Schema())
        for i, t in enumerate(self.build.Schema()):
            cfg.build_types[i] = t
        for i, t in enumerate(self.probe.Schema()):
            cfg.probe_types[i] = t
        cfg.max_chunk_size = 1024
        self.cfg, self.h, self.prepared = cfg, None, False
        self.pull_rows = (pull_rows + 7) & ~7
        self.out = None

    def Open(self):
        super().Open()
        h = C.c_void_p()
        _lib.check(self.lib.tsq_join_create(self.ctx.h, C.byref(self.cfg), C.byref(h)), self.ctx.h)
        self.h, self.prepared = h, False
        if self.used is not None:
            flags = (C.c_uint8 * len(self.types))(*[1 if i in self.used else 0 for i in range(len(self.types))])
            _lib.check(self.lib.tsq_join_set_used_columns(h, flags, len(self.types)), h)
        # fixed-width outputs are BORROWED from the operator's result batch (TSQ_COL_BORROW: pointers valid until the next pull) — the
        # device form of Chunk.SwapColumns; a var-len output column keeps the copying pull
        self.borrow = abi.BYTES not in self.types
        self.out = None if self.borrow else self._buffers(self.pull_rows)

    def Next(self):
        if not self.prepared:
            while True:
                chk = self.build.Next()
                if chk.NumRows() == 0:
                    break
                if chk.sel:  # tsq_join_build_push has no `selected`: flags on the build side would be ignored silently
                    raise ValueError("GpuHashJoinExec: selection flags on the build side: use GpuSelectionExec(compact=True)")
                _lib.check(self.lib.tsq_join_build_push(self.h, chk.cols(), len(chk.columns), chk.NumRows()), self.h)
            _lib.check(self.lib.tsq_join_build_finish(self.h), self.h)
            self.prepared = True
        n, eos = C.c_int64(0), C.c_int32(0)
        while True:
            if self.borrow:
                oc = (abi.Col * len(self.types))()
                for i, t in enumerate(self.types):
                    oc[i].type, oc[i].elem_size, oc[i].flags = t, _es(t), abi.COL_DEVICE | abi.COL_BORROW
                _lib.check(self.lib.tsq_join_pull(self.h, oc, len(self.types), self.pull_rows, C.byref(n), C.byref(eos)), self.h)
                if n.value > 0:
                    # a column the parent does not use has no data: it aliases a materialised column's buffer so that a consumer which
                    # passes whole chunks on (it never reads the cells) still hands out valid pointers
                    alias = next(oc[i].data for i in range(len(self.types)) if oc[i].data)
                    cols = [DeviceColumn(self.ctx, t, n.value, data=oc[i].data or alias, bitmap=oc[i].null_bitmap if oc[i].data else None) for i, t in enumerate(self.types)]
                    return DeviceChunk(cols, n.value)
            else:
                self._size_varlen(self.lib.tsq_join_peek, self.h, self.out, self.pull_rows)
                oc = (abi.Col * len(self.out))(*[c.col(self.pull_rows) for c in self.out])
                _lib.check(self.lib.tsq_join_pull(self.h, oc, len(self.out), self.pull_rows, C.byref(n), C.byref(eos)), self.h)
                if n.value > 0:
                    return DeviceChunk(self.out, n.value)
            if eos.value:
                return EOS
            chk = self.probe.Next()
            if chk.NumRows() == 0:
                _lib.check(self.lib.tsq_join_probe_finish(self.h), self.h)
                continue
            # a probe-side chunk may carry selection flags (GpuSelectionExec(compact=False)): the join takes them as `selected`.
            # Under an OUTER join a row with selected == 0 is emitted NULL-padded (onMissMatch, executor/join.go:344-345), not dropped:
            # flags are a WHERE filter only below an inner join — anything else must compact first
            if chk.sel and self.cfg.join_type != abi.JOIN_INNER:
                raise ValueError("GpuHashJoinExec: selection flags on the probe side of an outer join: use GpuSelectionExec(compact=True)")
            _lib.check(self.lib.tsq_join_probe_push(self.h, chk.cols(), len(chk.columns), chk.NumRows(), C.c_void_p(chk.sel) if chk.sel else None), self.h)

    def Close(self):
        if self.h:
            st = abi.Stats()
            if self.lib.tsq_join_stats(self.h, C.byref(st)) == abi.OK:
                self.last_stats = st  # which route the probe batches took (tools/q3.py reports it)
            self.lib.tsq_join_cancel(self.h)
            self.lib.tsq_join_destroy(self.h)
            self.h = None
        if self.out:
            for c in self.out:
                c.free()
            self.out = None
        super().Close()


class GpuHashAggExec(GpuExecutor):
    """HashAggExec on device-resident chunks (tsq_agg_*); stream=True: StreamAggExec — the child delivers its rows ordered by the group
    keys (a GpuSortExec, an ordered scan) and the groups come out in that order (tsq_agg_set_stream)."""

    def __init__(self, ctx, child, group_by_cols, agg_funcs, est_groups=0, pull_rows=1 << 22, stream=False):
        self.stream = stream
        types = []
        for f in agg_funcs:
            types += f.out_types()
        super().__init__(ctx, types, (child,))
        self.child = child
        cfg = abi.AggCfg()
        in_types = child.Schema()
        # more than four group-by columns: tsq_agg_create_keys, the keys beside the cfg (as executor.HashAggExec)
        self.many_keys = None
        if len(group_by_cols) > abi.MAX_GROUP_KEYS:
            self.many_keys = (list(group_by_cols), [in_types[c] for c in group_by_cols])
        else:
            cfg.n_group_keys = len(group_by_cols)
            for i, c in enumerate(group_by_cols):
                cfg.group_key_col[i], cfg.group_key_type[i] = c, in_types[c]
        cfg.n_aggs = len(agg_funcs)
        for i, f in enumerate(agg_funcs):
            cfg.aggs[i].func, cfg.aggs[i].mode = f.func, f.mode
            cfg.aggs[i].arg_col, cfg.aggs[i].arg_col2, cfg.aggs[i].arg_type = f.arg_col, f.arg_col2, f.arg_type
        cfg.n_input_cols = len(in_types)
        for i, t in enumerate(in_types):
            cfg.input_types[i] = t
        cfg.est_groups, cfg.max_chunk_size = est_groups, 1024
        self.cfg, self.h, self.prepared, self.out = cfg, None, False, None
        self.pull_rows = (pull_rows + 7) & ~7

    def Open(self):
        super().Open()
        h = C.c_void_p()
        if self.many_keys:
            kc, kt = self.many_keys
            _lib.check(self.lib.tsq_agg_create_keys(self.ctx.h, C.byref(self.cfg), (C.c_int32 * len(kc))(*kc), (C.c_int32 * len(kt))(*kt), len(kc), C.byref(h)),
                       self.ctx.h)
        else:
            _lib.check(self.lib.tsq_agg_create(self.ctx.h, C.byref(self.cfg), C.byref(h)), self.ctx.h)
        if self.stream:
            _lib.check(self.lib.tsq_agg_set_stream(h, 1), h)
        self.h, self.prepared = h, False
        self.out = self._buffers(self.pull_rows)

    def Next(self):
        if not self.prepared:
            self.pushed = False
            while True:
                chk = self.child.Next()
                if chk.NumRows() == 0:
                    break
                _lib.check(self.lib.tsq_agg_push(self.h, chk.cols(), len(chk.columns), chk.NumRows()), self.h)
                self.pushed = True
            _lib.check(self.lib.tsq_agg_finish(self.h), self.h)
            self.prepared = True
        if not self.pushed:
            # no input chunk: GROUP BY yields no rows (aggregate_test.go:58-59).  The single default row of a key-less
            # aggregate over empty input (aggregate.go:572-574) is served by the host-chunk HashAggExec.
            return EOS
        n, eos = C.c_int64(0), C.c_int32(0)
        self._size_varlen(self.lib.tsq_agg_peek, self.h, self.out, self.pull_rows)
        oc = (abi.Col * len(self.out))(*[c.col(self.pull_rows) for c in self.out])
        _lib.check(self.lib.tsq_agg_pull(self.h, oc, len(self.out), self.pull_rows, C.byref(n), C.byref(eos)), self.h)
        if n.value == 0:
            return EOS
        return DeviceChunk(self.out, n.value)

    def Close(self):
        if self.h:
            self.lib.tsq_agg_cancel(self.h)
            self.lib.tsq_agg_destroy(self.h)
            self.h = None
        if self.out:
            for c in self.out:
                c.free()
            self.out = None
        super().Close()


class GpuSortExec(GpuExecutor):
    """SortExec / TopNExec on device-resident chunks: tsq_sort_* with TSQ_COL_DEVICE columns (executor/sort.go:27-318)."""

    def __init__(self, ctx, child, by_cols, by_desc, offset=0, count=-1, pull_rows=1 << 22):
        super().__init__(ctx, child.Schema(), (child,))
        self.child = child
        cfg = abi.SortCfg()
        cfg.n_cols = len(self.types)
        for i, t in enumerate(self.types):
            cfg.col_types[i] = t
        cfg.n_keys = len(by_cols)
        for i, (c, d) in enumerate(zip(by_cols, by_desc)):
            cfg.key_col[i], cfg.key_desc[i] = c, 1 if d else 0
        cfg.limit_offset, cfg.limit_count, cfg.max_chunk_size = offset, count, 1024
        self.cfg, self.h, self.fetched, self.out = cfg, None, False, None
        self.pull_rows = (pull_rows + 7) & ~7

    def Open(self):
        super().Open()
        h = C.c_void_p()
        _lib.check(self.lib.tsq_sort_create(self.ctx.h, C.byref(self.cfg), C.byref(h)), self.ctx.h)
        self.h, self.fetched = h, False
        self.out = self._buffers(self.pull_rows)

    def Next(self):
        if not self.fetched:
            while True:
                chk = self.child.Next()
                if chk.NumRows() == 0:
                    break
                _lib.check(self.lib.tsq_sort_push(self.h, chk.cols(), len(chk.columns), chk.NumRows()), self.h)
            _lib.check(self.lib.tsq_sort_finish(self.h), self.h)
            self.fetched = True
        n, eos = C.c_int64(0), C.c_int32(0)
        self._size_varlen(self.lib.tsq_sort_peek, self.h, self.out, self.pull_rows)
        oc = (abi.Col * len(self.out))(*[c.col(self.pull_rows) for c in self.out])
        _lib.check(self.lib.tsq_sort_pull(self.h, oc, len(self.out), self.pull_rows, C.byref(n), C.byref(eos)), self.h)
        return DeviceChunk(self.out, n.value) if n.value else EOS

    def Close(self):
        if self.h:
            self.lib.tsq_sort_cancel(self.h)
            self.lib.tsq_sort_destroy(self.h)
            self.h = None
        if self.out:
            for c in self.out:
                c.free()
            self.out = None
        super().Close()


class _OneChunk(GpuExecutor):
    """a device chunk as a child executor: handed out once"""

    def __init__(self, ctx, chunk):
        super().__init__(ctx, chunk.types())
        self.chunk, self.done = chunk, False

    def Next(self):
        if self.done:
            return EOS
        self.done = True
        return self.chunk


def unionscan_set_added(ctx, handle, added_rows, conditions):
    """tsq_unionscan_set_added with the transaction's added rows (a host Chunk or a DeviceChunk, in scan order).  `conditions` are applied
    first through the filter path of the library (tsq_filter_eval + tsq_chunk_compact: GpuSelectionExec), which is the mem readers'
    EvalBool loop (mem_reader.go:188-213); the rows keep their order."""
    lib, own = ctx.lib, None
    chk = added_rows
    if isinstance(chk, Chunk):
        if chk.NumRows() == 0 or not conditions:
            keep = []
            from .chunk import make_cols
            _lib.check(lib.tsq_unionscan_set_added(handle, make_cols(chk.columns, keep), len(chk.columns), chk.NumRows()), handle)
            return
        chk = own = DeviceChunk.from_host(ctx, chk)
    sel = None
    try:
        if conditions and chk.NumRows():
            sel = GpuSelectionExec(ctx, _OneChunk(ctx, chk), conditions)
            sel.Open()
            chk = sel.Next()
        _lib.check(lib.tsq_unionscan_set_added(handle, chk.cols() if chk.NumRows() else None, len(chk.columns), chk.NumRows()), handle)
    finally:
        if sel:
            sel.Close()
        if own:
            own.free()


def _owned_rows(ctx, exe):
    """Open / Next* / Close of a device executor -> ONE DeviceChunk that owns its columns (with null bitmaps), the rows in their order"""
    out = None
    exe.Open()
    try:
        while True:
            chk = exe.Next()
            if chk.NumRows() == 0:
                break
            if out is None:
                out = DeviceChunk([DeviceColumn(ctx, c.tp, max(chk.NumRows(), 8), cap_bytes=c.nbytes(chk.NumRows()) + 8 if c.var else 0) for c in chk.columns], 0)
            out.append(ctx, chk)
    except Exception:
        if out:
            out.free()
        raise
    finally:
        exe.Close()
    return out if out else DeviceChunk([DeviceColumn(ctx, t, 8, cap_bytes=8 if t == abi.BYTES else 0) for t in exe.Schema()], 0)


def _filter_rows(ctx, chunk, conditions):
    """the mem readers' EvalBool loop over an owned chunk (tsq_filter_eval + tsq_chunk_compact: GpuSelectionExec); the rows keep their
    order; `chunk` is freed when a filtered copy takes its place"""
    if not conditions or chunk.NumRows() == 0:
        return chunk
    try:
        return _owned_rows(ctx, GpuSelectionExec(ctx, _OneChunk(ctx, chunk), conditions))
    finally:
        chunk.free()


def memTableReader(ctx, membuf, columns, kvRanges, desc=False, conditions=None, point_keys=None):
    """memTableReader.getMemRows (executor/mem_reader.go:188-221) on the device: tsq_membuf_scan over the reader's ranges ->
    tsq_rowkeys_decode -> tsq_rowcodec_decode with the reader's rowcodec.ColInfos (the handle column included) -> the conditions.
    -> a DeviceChunk of the transaction's added rows in scan order, which the caller frees.  PINNED DEPARTURE: all rows are decoded, then
    filtered — a decode error behind an earlier condition error wins; the statement fails either way."""
    from .coprocessor import tableScanExec
    n = max(int(membuf.Len()), 8)
    e = tableScanExec.from_membuffer(ctx, columns, membuf, kvRanges, desc, batch_rows=n, point_keys=point_keys)
    return _filter_rows(ctx, _owned_rows(ctx, e), conditions)


def memIndexReader(ctx, membuf, types, pkStatus, outputOffset, kvRanges, desc=False, conditions=None):
    """memIndexReader.getMemRows (mem_reader.go:67-130): tsq_membuf_scan -> tsq_indexkeys_decode (types: the index columns' and, last, the
    handle's; pkStatus 2 = PrimaryKeyIsUnsigned; the handle comes from the key, or from the value for a unique index) -> the columns at
    outputOffset -> the conditions.  -> a DeviceChunk in scan order, which the caller frees."""
    from .coprocessor import indexScanExec
    assert pkStatus in (indexScanExec.PrimaryKeyIsSigned, indexScanExec.PrimaryKeyIsUnsigned) and len(set(outputOffset)) == len(outputOffset)
    e = indexScanExec.from_membuffer(ctx, types, len(types) - 1, pkStatus, membuf, kvRanges, desc, batch_rows=max(int(membuf.Len()), 8))
    rows = _owned_rows(ctx, e)
    for i, c in enumerate(rows.columns):
        if i not in outputOffset:
            c.free()
    return _filter_rows(ctx, DeviceChunk([rows.columns[o] for o in outputOffset], rows.NumRows()), conditions)


def memIndexLookUpReader(ctx, membuf, types, pkStatus, table_id, columns, kvRanges, desc=False, conditions=None):
    """memIndexLookUpReader.getMemRows (mem_reader.go:359-398): the index scan's handle column alone (getMemRowsHandle, reversed for
    desc) -> tsq_rowkeys_encode -> tsq_membuf_scan_points (one point per handle, in the index's order; the table side is not reversed a
    second time) -> the table decode and the conditions.  The handles never leave the device."""
    handles = memIndexReader(ctx, membuf, types, pkStatus, [len(types) - 1], kvRanges, desc)
    keys = None
    try:
        n = handles.NumRows()
        keys = ctx.alloc(max(n, 1) * 19 + 64)
        if n:
            _lib.check(ctx.lib.tsq_rowkeys_encode(ctx.h, table_id, C.c_void_p(handles.columns[0].data), n, abi.COL_DEVICE, C.c_void_p(keys)), ctx.h)
        return memTableReader(ctx, membuf, columns, None, False, conditions, point_keys=(keys, n))
    finally:
        handles.free()
        if keys:
            ctx.free(keys)


class GpuUnionScanExec(GpuExecutor):
    """UnionScanExec on device-resident chunks (tsq_unionscan_* with TSQ_COL_DEVICE columns, executor/union_scan.go:89-300): sits on a
    GPU reader (coprocessor.tableScanExec / indexScanExec output) and under GpuHashJoinExec / GpuHashAggExec; nothing is copied to the
    host.  dirty: executor.DirtyTable; added_rows: a DeviceChunk or host Chunk in scan order."""

    def __init__(self, ctx, child, dirty, added_rows, used_index, below_handle_index, desc, conditions=None, pull_rows=1 << 22):
        super().__init__(ctx, child.Schema(), (child,))
        from .executor import unionscan_cfg
        self.child, self.dirty, self.added_rows, self.conditions = child, dirty, added_rows, list(conditions or [])
        self.cfg = unionscan_cfg(self.types, used_index, below_handle_index, desc, 1024)
        self.h, self.out = None, None
        self.pull_rows = (pull_rows + 7) & ~7

    membuf = None  # from_membuffer: (kv.MemBuffer, table id, reader)

    @classmethod
    def from_membuffer(cls, ctx, child, membuf, table_id, reader, used_index, below_handle_index, desc, conditions=None, pull_rows=1 << 22):
        """read your own writes without the host: at Open the table's dirty handles come out of the finished kv.MemBuffer
        (tsq_membuf_dirty) into tsq_unionscan_create_dev, and `reader` — a callable without arguments that returns the added rows
        as a DeviceChunk in scan order, unfiltered: memTableReader / memIndexReader / memIndexLookUpReader over the same buffer —
        feeds tsq_unionscan_set_added through `conditions`.  Nothing of the buffer crosses to the host but counts."""
        e = cls(ctx, child, None, None, used_index, below_handle_index, desc, conditions, pull_rows)
        e.membuf = (membuf, table_id, reader)
        return e

    def _open_membuffer(self):
        membuf, table_id, reader = self.membuf
        ctx = self.ctx
        added, n_added, deleted, n_deleted = membuf.dirty_handles(table_id)
        try:
            h = C.c_void_p()
            _lib.check(self.lib.tsq_unionscan_create_dev(ctx.h, C.byref(self.cfg), C.c_void_p(added), n_added, C.c_void_p(deleted), n_deleted, C.byref(h)), ctx.h)
            self.h = h
        finally:  # (the set is built when the call returns)
            ctx.free(added)
            ctx.free(deleted)
        rows = reader()
        try:
            unionscan_set_added(ctx, self.h, rows, self.conditions)
        finally:
            rows.free()

    def Open(self):
        super().Open()
        if self.membuf:
            self._open_membuffer()
        else:
            from .executor import unionscan_create
            self.h = unionscan_create(self.ctx, self.cfg, self.dirty)
            unionscan_set_added(self.ctx, self.h, self.added_rows, self.conditions)
        self.out = self._buffers(self.pull_rows)

    def Next(self):
        while True:
            n, eos = C.c_int64(0), C.c_int32(0)
            self._size_varlen(self.lib.tsq_unionscan_peek, self.h, self.out, self.pull_rows)
            oc = (abi.Col * len(self.out))(*[c.col(self.pull_rows) for c in self.out])
            _lib.check(self.lib.tsq_unionscan_pull(self.h, oc, len(self.out), self.pull_rows, C.byref(n), C.byref(eos)), self.h)
            if n.value:
                return DeviceChunk(self.out, n.value)
            if eos.value:
                return EOS
            chk = self.child.Next()  # more input is needed: one child chunk, or the end
            if chk.NumRows() == 0:
                _lib.check(self.lib.tsq_unionscan_finish(self.h), self.h)
            else:
                _lib.check(self.lib.tsq_unionscan_push(self.h, chk.cols(), len(chk.columns), chk.NumRows()), self.h)

    def stats(self):
        a, b, c, ms = C.c_int64(0), C.c_int64(0), C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_unionscan_stats(self.h, C.byref(a), C.byref(b), C.byref(c), C.byref(ms)), self.h)
        return {"snapshot_rows": a.value, "dropped_rows": b.value, "added_rows_out": c.value, "kernel_ms": ms.value}

    def Close(self):
        if self.h:
            self.lib.tsq_unionscan_cancel(self.h)
            self.lib.tsq_unionscan_destroy(self.h)
            self.h = None
        if self.out:
            for c in self.out:
                c.free()
            self.out = None
        super().Close()


class GpuIndexLookUpExecutor(GpuExecutor):
    """IndexLookUpExecutor, the double read (executor/distsql.go:237-637), on device chunks.  index_child: any GpuExecutor whose LAST
    column is the handle (a coprocessor.indexScanExec, optionally under selectionExec / limitExec): the index worker.  table: a
    coprocessor.DeviceTable; columns: the table scan's rowcodec.ColInfos; tbl_conditions: the table-side conditions (tblPlans).
    Tasks are cut as indexWorker.extractTaskHandles does (:510-535): a task holds exactly batchSize handles except the last one,
    batchSize starts at min(init_batch_size, max_batch_size) and doubles after each full task up to max_batch_size — the child's
    device chunks are sliced, not rounded to chunk boundaries.  Per task coprocessor.tableLookupExec reads the rows, then the
    conditions run (tsq_filter_eval + tsq_chunk_compact, as selectionExec); tasks are emitted in order (resultCh), one chunk per
    task that has rows.  keep_order: rows in index order, else in handle order within a task.  The handles never leave HBM."""

    def __init__(self, ctx, index_child, table, columns, tbl_conditions, keep_order, init_batch_size, max_batch_size):
        from .coprocessor import tableLookupExec
        self.reader = tableLookupExec(ctx, table, columns, keep_order)
        super().__init__(ctx, self.reader.Schema(), (index_child,))
        if index_child.Schema()[-1] not in (abi.I64, abi.U64):
            raise Unsupported("GpuIndexLookUpExecutor: the last column of the index side must be the handle (an 8-byte integer column)")
        if int(max_batch_size) < 1 or int(init_batch_size) < 1:
            raise ValueError("GpuIndexLookUpExecutor: batch sizes must be positive")
        self.index_child, self.table = index_child, table
        self.conditions = list(tbl_conditions or [])
        self.init_batch, self.max_batch = int(init_batch_size), int(max_batch_size)
        self.top = GpuSelectionExec(ctx, self.reader, self.conditions) if self.conditions else self.reader
        self.task_buf, self.task_cap = None, 0
        self.task_sizes = []  # handles per task, in order (tests, the bench tool)

    def Open(self):
        super().Open()
        self.top.Open()
        self.batch = min(self.init_batch, self.max_batch)
        self.cur, self.cur_pos, self.index_done = None, 0, False
        self.task_sizes = []

    def _fill_task(self):
        """the next task's handles -> self.task_buf; returns their number (0: the index side is exhausted)"""
        want, have = self.batch, 0
        if want > self.task_cap:
            if self.task_buf:
                self.ctx.free(self.task_buf)
            self.task_cap = want
            self.task_buf = self.ctx.alloc(want * 8 + 64)
        while have < want and not self.index_done:
            if self.cur is None or self.cur_pos >= self.cur.NumRows():
                chk = self.index_child.Next()
                if chk.NumRows() == 0:
                    self.index_done, self.cur = True, None
                    break
                self.cur, self.cur_pos = chk, 0
            take = min(want - have, self.cur.NumRows() - self.cur_pos)
            hcol = self.cur.columns[-1]
            _lib.check(self.lib.tsq_copy_d2d(self.ctx.h, C.c_void_p(self.task_buf + 8 * have), C.c_void_p(hcol.data + 8 * self.cur_pos), 8 * take), self.ctx.h)
            have += take
            self.cur_pos += take
        if have == want:  # a full task: the next one may be twice as large (distsql.go:530-533)
            self.batch = min(self.batch * 2, self.max_batch)
        return have

    def Next(self):
        while True:
            n = self._fill_task()
            if n == 0:
                return EOS
            self.task_sizes.append(n)
            self.reader.set_task(self.task_buf, n)
            chk = self.top.Next()
            if chk.NumRows():
                return chk

    def Close(self):
        self.top.Close()  # (the selection closes the reader, its child)
        if self.task_buf:
            self.ctx.free(self.task_buf)
        self.task_buf, self.task_cap = None, 0
        super().Close()


class InsertTableInfo:
    """the part of model.TableInfo an INSERT reads: ID, Columns (table.ColumnInfo, in Table.Cols() order), ColumnIDs, PKIsHandle with the
    offset of the primary-key column, and the offset of the auto-increment column (-1: none)"""

    def __init__(self, ID, Columns, ColumnIDs, PKIsHandle=False, pk_offset=-1):
        from .table import AutoIncrementFlag
        self.ID, self.Columns, self.ColumnIDs, self.PKIsHandle, self.pk_offset = ID, list(Columns), list(ColumnIDs), PKIsHandle, pk_offset
        auto = [i for i, c in enumerate(self.Columns) if c.Flag & AutoIncrementFlag]
        self.auto_offset = auto[0] if auto else -1


class InsertIndexInfo:
    """model.IndexInfo: ID, Unique, the offsets of its columns in the table"""

    def __init__(self, ID, Unique, Columns):
        self.ID, self.Unique, self.Columns = ID, Unique, list(Columns)


class InsertBatch:
    """the KV pairs of one chunk of the select, in HBM: record keys (19 bytes each), stored rows (rowcodec.DeviceBytes), and per
    index a tablecodec.DeviceIndexKVs; `rows` = the cast chunk itself.  The caller writes them through its transaction and frees the batch"""

    def __init__(self, ctx, n, rows, row_keys, row_values, index_kvs, handles, own_handles):
        self.ctx, self.n, self.rows, self.row_keys, self.row_values, self.index_kvs = ctx, n, rows, row_keys, row_values, index_kvs
        self.handles, self._own_handles = handles, own_handles

    def to_host(self):
        """(record keys [n, 19], (row values, offsets), [index (keys, key_offsets, values, value_offsets, distinct)])"""
        keys = np.zeros(max(self.n, 1) * 19, np.uint8)
        if self.n:
            self.ctx.d2h(keys, self.row_keys)
        return keys[:self.n * 19].reshape(self.n, 19), self.row_values.to_host(), [k.to_host() for k in self.index_kvs]

    def write_to(self, membuf):
        """what tables.AddRecord does with its transaction (table/tables/tables.go:484-526: txn.Set of the record, index.Create's Set per
        index), into a kv.MemBuffer: the record keys with the stored rows, then the keys and values of every index — device arrays, copied
        by the push, nothing leaves HBM.  (An index stream's value bytes are pushed by their capacity, 8 per row: the offsets say what of
        them is a value.)  The batch may be freed afterwards."""
        n = self.n
        if n == 0:
            return
        membuf.set_packed(self.row_keys, None, n * 19, n, self.row_values.p, self.row_values.offsets, self.row_values.nbytes, device=True)
        for k in self.index_kvs:
            membuf.set_packed(k.keys, k.key_offsets, k.nbytes, n, k.values, k.value_offsets, n * 8, device=True)

    def free(self):
        self.rows.free()
        self.row_values.free()
        for k in self.index_kvs:
            k.free()
        self.ctx.free(self.row_keys)
        if self._own_handles:
            self.ctx.free(self.handles)
        self.row_keys = self.handles = None


class GpuInsertSelectExec(GpuExecutor):
    """INSERT .. SELECT (insertRowsFromSelect, executor/insert_common.go:340-381) on device chunks: per chunk of the child getRow's casts,
    defaults and NOT NULL checks (tsq_cast_run), the auto-increment ids (tsq_autoid_fill), then what tables.AddRecord computes — the
    record keys, the stored rows, the entries of every index.  insertColumns[i] = the offset of the table column the child's column i
    goes to.  The handle is the primary-key column when table.PKIsHandle, otherwise rowid_base + 1, + 2, ... (the _tidb_rowid
    allocator; the caller passes its base).  Next() returns an InsertBatch, or None at the end; afterwards rowCount, lastInsertID,
    insertID, autoid_base (what the shim rebases the allocator to, once), rowid_base and warnings tell the statement's outcome.
    The first failing cell raises table.CastError (.row counts from the start of the statement) or table.AutoIDError.
    store = (coprocessor.DeviceTable, [coprocessor.DeviceIndex per UNIQUE index of `indices`, in their order]): the duplicate-key check
    of tables.AddRecord (table/tables/tables.go:528-581) runs on the device too (dupcheck.DupChecker, INSERT mode).  The select then runs
    to its end before the first batch is handed out — every chunk's keys are pushed, the statement is checked once, and a conflict raises
    dupcheck.KeyExistsError(row, stream, dup_handle) with no batch handed out; the batches wait in HBM meanwhile, so a statement of more than
    max_rows rows raises abi.ERR_UNSUPPORTED (the shim runs the Go operator).  DEPARTURE in error order: the reference adds the rows of a
    chunk before it casts the next one (insert_common.go:355-379), so its ErrKeyExists of an early chunk comes before a cast or auto-id
    error of a later chunk; here every chunk is cast first and the later chunk's CastError / AutoIDError is what the statement raises.
    Either way the statement fails and writes nothing.  store = None: no check, batch by batch as before.  What stays with the host then: the duplicate-key look-ups in the store; in both cases the locks and the
    transaction."""

    def __init__(self, ctx, child, table, insertColumns, indices, stmt, autoid_base=0, rowid_base=0, store=None, max_rows=1 << 24):
        super().__init__(ctx, [], (child,))
        self.store, self._held, self._checked, self.max_rows = store, [], False, max_rows
        from .table import Caster
        self.child, self.table, self.indices, self.stmt = child, table, list(indices), stmt
        src_cols = [-1] * len(table.Columns)
        for i, off in enumerate(insertColumns):
            src_cols[off] = i
        self.caster = Caster(ctx, table.Columns, src_cols, child.Schema(), stmt)
        self.src_cols = src_cols
        self.autoid_base, self.rowid_base = autoid_base, rowid_base
        self.rowCount, self.lastInsertID, self.insertID = 0, 0, 0
        self.warnings = self.caster.warnings
        # tables.AddRecord leaves the PK-handle column out of the row value (table/tables/tables.go:474-481)
        self.row_cols = [i for i in range(len(table.Columns)) if not (table.PKIsHandle and i == table.pk_offset)]

    def _fill_ids(self, col, n):
        from .table import FillAutoID
        _, nb, first, last = FillAutoID(self.ctx, col, n, self.autoid_base, self.table.Columns[self.table.auto_offset], self.stmt)
        self.autoid_base = nb
        if self.lastInsertID == 0:
            self.lastInsertID = first
        if last:
            self.insertID = last

    def _check_statement(self):
        """with a store: the whole select, its keys pushed chunk by chunk, then the one verdict"""
        from . import dupcheck as D
        table, unique = self.store
        uix = [k for k, ix in enumerate(self.indices) if ix.Unique]
        assert len(unique) == len(uix), "store: one DeviceIndex per unique index"
        streams = [D.HandleStream(*table.handles())] if self.table.PKIsHandle else []
        for k, di in zip(uix, unique):
            cols = self.indices[k].Columns
            streams.append(D.IndexStream(di.keys.p, di.key_offsets.p, di.key_bytes, di.handles.p, di.n,
                                         float_key=any(self.table.Columns[c].Tp in (abi.TP_FLOAT, abi.TP_DOUBLE) for c in cols)))
        if not streams:
            return
        base0 = self.rowid_base
        th, tn = (None, 0) if self.table.PKIsHandle else table.handles()
        chk = D.DupChecker(self.ctx, streams, abi.DUP_INSERT, th, tn)
        starts = []
        try:
            while True:
                b = self._next_batch()
                if b is None:
                    break
                starts.append(self.rowCount - b.n)
                self._held.append(b)
                if self.rowCount > self.max_rows:
                    raise _lib.TsqError(abi.ERR_UNSUPPORTED, "INSERT .. SELECT with a store: more than max_rows rows in one statement")
                keys = [b.handles] if self.table.PKIsHandle else []
                keys += [(b.index_kvs[k].keys, b.index_kvs[k].key_offsets, b.index_kvs[k].nbytes, b.index_kvs[k].distinct) for k in uix]
                chk.push(keys, b.n)
            err = chk.match_insert()
            if err is not None and not err.from_store:  # the entry the FIRST row of the key's group wrote: that row's handle
                if self.table.PKIsHandle:
                    at = max(i for i, s0 in enumerate(starts) if s0 <= err.dup_row)
                    one = np.zeros(1, np.int64)
                    self.ctx.d2h(one, self._held[at].handles + 8 * (err.dup_row - starts[at]))
                    h = int(one[0])
                else:
                    h = base0 + err.dup_row + 1
                err = D.KeyExistsError(err.row, err.stream, h, False, err.dup_row)
            if err is not None:
                raise err
        except Exception:
            for b in self._held:
                b.free()
            self._held = []
            raise
        finally:
            chk.close()

    def Next(self):
        if self.store is None:
            return self._next_batch()
        if not self._checked:
            self._checked = True
            self._check_statement()
        return self._held.pop(0) if self._held else None

    def _next_batch(self):
        from . import rowcodec, tablecodec
        from .table import AutoIDError, CastError
        chk = self.child.Next()
        n = chk.NumRows()
        if n == 0:
            return None
        auto = self.table.auto_offset
        try:
            rows = self.caster.run(chk, partial=True)
        except CastError as e:
            # fillRow gives the ids row by row: an id that leaves its column's range in an EARLIER row (or in this row, in front of the
            # NOT NULL failure of a later column) is the statement's error instead
            part = e.partial
            try:
                if auto >= 0 and part is not None:
                    m = e.row + (1 if e.status == abi.ERR_BAD_NULL and auto < e.column else 0)
                    if m > 0:
                        try:
                            self._fill_ids(part.columns[auto], m)
                        except AutoIDError as a:
                            if a.row >= 0:
                                a.row += self.rowCount
                            raise a from None
            finally:
                if part is not None:
                    part.free()
            e.row += self.rowCount
            raise
        try:
            if auto >= 0:
                try:
                    self._fill_ids(rows.columns[auto], n)
                except AutoIDError as a:
                    if a.row >= 0:
                        a.row += self.rowCount
                    raise
            if self.table.PKIsHandle:
                handles, own = rows.columns[self.table.pk_offset].data, False
            else:
                handles, own = self.ctx.alloc(n * 8 + 64), True
                spec = abi.GenSpec()
                spec.kind, spec.start = abi.GEN_SEQ, self.rowid_base + 1
                self.ctx.gen_column(spec, n, handles)
                self.rowid_base += n
        except Exception:
            rows.free()
            raise
        keys = row_values = None
        kvs = []
        try:
            keys = self.ctx.alloc(n * 19 + 64)
            _lib.check(self.lib.tsq_rowkeys_encode(self.ctx.h, self.table.ID, C.c_void_p(handles), n, abi.COL_DEVICE, C.c_void_p(keys)), self.ctx.h)
            row_values = rowcodec.Encoder().Encode(self.ctx, DeviceChunk([rows.columns[i] for i in self.row_cols], n), [self.table.ColumnIDs[i] for i in self.row_cols])
            for ix in self.indices:
                kvs.append(tablecodec.GenIndexKeys(self.ctx, self.table.ID, ix.ID, ix.Unique, DeviceChunk([rows.columns[i] for i in ix.Columns], n), handles))
        except Exception:
            for k in kvs:
                k.free()
            if row_values is not None:
                row_values.free()
            if keys:
                self.ctx.free(keys)
            if own:
                self.ctx.free(handles)
            rows.free()
            raise
        self.rowCount += n
        return InsertBatch(self.ctx, n, rows, keys, row_values, kvs, handles, own)

    def Close(self):
        for b in self._held:
            b.free()
        self._held = []
        if self.caster:
            self.caster.close()
            self.caster = None
        super().Close()


class GpuDeleteExec(GpuExecutor):
    """DELETE over device chunks: deleteSingleTableByChunk (executor/delete.go) with what TableCommon.RemoveRecord computes per row
    (table/tables/tables.go:652-714) — the record key of the row's handle and, for every index, the key index.GenIndexKey gives for the
    index's columns of the row (a unique index with a NULL cell takes the handle-suffixed key: the encoder decides) — pushed into the
    transaction buffer `membuf` (kv.MemBuffer) as one DELETE push per stream and chunk.  The child hands out the table's columns in
    Table.Cols() order (what the index offsets refer to) with the handle at handle_ordinal.  Next() returns no rows; after Close() the
    buffer holds the statement and affectedRows counts its rows.  Nothing of a key leaves HBM.  The deleted handles are not recorded in
    an executor.DirtyTable: they reach the union scan through the buffer itself (tsq_membuf_dirty, GpuUnionScanExec.from_membuffer)."""

    def __init__(self, ctx, child, table, indices, handle_ordinal, membuf):
        super().__init__(ctx, [], (child,))
        self.child, self.table, self.indices, self.handle_ordinal, self.membuf = child, table, list(indices), handle_ordinal, membuf
        self.affectedRows = 0

    def Open(self):
        super().Open()
        self.affectedRows = 0

    def Next(self):
        from . import tablecodec
        while True:
            chk = self.child.Next()
            n = chk.NumRows()
            if n == 0:
                return EOS
            handles = chk.columns[self.handle_ordinal].data
            keys = self.ctx.alloc(n * 19 + 64)
            kvs = []
            try:
                _lib.check(self.lib.tsq_rowkeys_encode(self.ctx.h, self.table.ID, C.c_void_p(handles), n, abi.COL_DEVICE, C.c_void_p(keys)), self.ctx.h)
                for ix in self.indices:
                    kvs.append(tablecodec.GenIndexKeys(self.ctx, self.table.ID, ix.ID, ix.Unique, DeviceChunk([chk.columns[i] for i in ix.Columns], n), handles))
                self.membuf.delete_packed(keys, None, n * 19, n, device=True)
                for k in kvs:
                    self.membuf.delete_packed(k.keys, k.key_offsets, k.nbytes, n, device=True)
            finally:
                for k in kvs:
                    k.free()
                self.ctx.free(keys)
            self.affectedRows += n


class ReplaceBatch:
    """the outcome of one REPLACE .. SELECT, in HBM: the deletions (n_removed stored rows: their record keys and, per index of the table,
    a tablecodec.DeviceIndexKVs whose KEYS are deleted), the puts (an InsertBatch of the n_put rows that are written), `affected`
    (the reference's affected-rows count) and the _tidb_rowid base after the statement.  The caller applies the deletions, then the puts,
    through its transaction and frees the batch."""

    def __init__(self, ctx, n_removed, del_keys, del_index_kvs, removed_handles, puts, affected, rowid_base, n_rows):
        self.ctx, self.n_removed, self.del_keys, self.del_index_kvs, self.removed_handles = ctx, n_removed, del_keys, del_index_kvs, removed_handles
        self.puts, self.affected, self.rowid_base, self.n_rows = puts, affected, rowid_base, n_rows

    def to_host(self):
        """(deleted record keys [n_removed, 19], [per index the deleted (keys, key_offsets)], the puts as InsertBatch.to_host gives them or None)"""
        keys = np.zeros(max(self.n_removed, 1) * 19, np.uint8)
        if self.n_removed:
            self.ctx.d2h(keys, self.del_keys)
        return (keys[:self.n_removed * 19].reshape(self.n_removed, 19), [k.to_host()[:2] for k in self.del_index_kvs],
                self.puts.to_host() if self.puts is not None else None)

    def free(self):
        for k in self.del_index_kvs:
            k.free()
        for p in (self.del_keys, self.removed_handles):
            if p:
                self.ctx.free(p)
        self.del_keys = self.removed_handles = None
        if self.puts is not None:
            self.puts.free()
            self.puts = None


class GpuReplaceSelectExec(GpuInsertSelectExec):
    """REPLACE .. SELECT (ReplaceExec, executor/replace.go:53-196) on device chunks.  The select runs to its end — the casts and auto ids per
    chunk as GpuInsertSelectExec does them, the cast rows appended to ONE device chunk (DeviceChunk.append) — then the statement is settled at
    once: the keys of every stream (PK handle, unique indexes) are pushed to a dupcheck.DupChecker in REPLACE mode, the old rows of the stored
    candidates come through coprocessor.tableLookupExec (lookup -> gather -> decode), tsq_rows_equal answers EqualDatums against the
    statement's own rows and against the old rows, and resolve names the rows that are written and the stored rows that go.
    store = (coprocessor.DeviceTable, [coprocessor.DeviceIndex per UNIQUE index, in their order]).  Next() returns ONE ReplaceBatch, then
    None.  Refusals (abi.ERR_UNSUPPORTED, the shim runs the Go operator): a statement of more than max_rows rows, a unique index over a
    FLOAT / DOUBLE column, and everything tsq_cast_create refuses.  What stays with the host: the locks, the transaction, applying the batch.
    The compaction of the stored candidates' handles (a list of at most n indices) is a host pass over two read-back arrays."""

    def __init__(self, ctx, child, table, insertColumns, indices, stmt, store, autoid_base=0, rowid_base=0, max_rows=1 << 24):
        for ix in indices:
            if ix.Unique and any(table.Columns[c].Tp in (abi.TP_FLOAT, abi.TP_DOUBLE) for c in ix.Columns):
                raise _lib.TsqError(abi.ERR_UNSUPPORTED, "REPLACE over a unique index with a FLOAT / DOUBLE column")
        super().__init__(ctx, child, table, insertColumns, indices, stmt, autoid_base=autoid_base, rowid_base=rowid_base)
        self.rstore, self.max_rows, self._done = store, max_rows, False
        self.affected = 0

    def _cast_chunk(self):
        """the next chunk of the select, cast, with its auto ids: a DeviceChunk the caller frees, or None"""
        from .table import AutoIDError, CastError
        chk = self.child.Next()
        n = chk.NumRows()
        if n == 0:
            return None
        try:
            rows = self.caster.run(chk)
        except CastError as e:
            e.row += self.rowCount
            raise
        try:
            if self.table.auto_offset >= 0:
                try:
                    self._fill_ids(rows.columns[self.table.auto_offset], n)
                except AutoIDError as a:
                    if a.row >= 0:
                        a.row += self.rowCount
                    raise
        except Exception:
            rows.free()
            raise
        self.rowCount += n
        return rows

    def _old_columns(self):
        from . import rowcodec as RC
        t = self.table
        return [RC.ColInfo(t.ColumnIDs[i], c.Tp, Flag=c.Flag, IsPKHandle=t.PKIsHandle and i == t.pk_offset, Flen=max(c.Flen, 0)) for i, c in enumerate(t.Columns)]

    def _encode(self, chunk, n, handles, own):
        """record keys, stored rows and index entries of a device chunk's rows: an InsertBatch"""
        from . import rowcodec, tablecodec
        keys = self.ctx.alloc(n * 19 + 64)
        _lib.check(self.lib.tsq_rowkeys_encode(self.ctx.h, self.table.ID, C.c_void_p(handles), n, abi.COL_DEVICE, C.c_void_p(keys)), self.ctx.h)
        row_values = rowcodec.Encoder().Encode(self.ctx, DeviceChunk([chunk.columns[i] for i in self.row_cols], n), [self.table.ColumnIDs[i] for i in self.row_cols])
        kvs = [tablecodec.GenIndexKeys(self.ctx, self.table.ID, ix.ID, ix.Unique, DeviceChunk([chunk.columns[i] for i in ix.Columns], n), handles) for ix in self.indices]
        return InsertBatch(self.ctx, n, chunk, keys, row_values, kvs, handles, own)

    def Next(self):
        from . import dupcheck as D
        from . import tablecodec
        from .coprocessor import tableLookupExec
        if self._done:
            return None
        self._done = True
        ctx, t = self.ctx, self.table
        dtable, unique = self.rstore
        uix = [ix for ix in self.indices if ix.Unique]
        assert len(unique) == len(uix), "store: one DeviceIndex per unique index"
        free, allc = [], None  # device blocks / objects to give back whatever happens

        def dev(nbytes):
            p = ctx.alloc(nbytes + 64)
            free.append(p)
            return p
        chk = look = None
        kvs = []
        try:
            # 1. the select to its end
            while True:
                rows = self._cast_chunk()
                if rows is None:
                    break
                if self.rowCount > self.max_rows:
                    rows.free()
                    raise _lib.TsqError(abi.ERR_UNSUPPORTED, "REPLACE .. SELECT: more than max_rows rows in one statement")
                if allc is None:
                    allc = rows
                else:
                    try:
                        allc.append(ctx, rows)
                    finally:
                        rows.free()
            n = self.rowCount
            if n == 0:
                return ReplaceBatch(ctx, 0, None, [], None, None, 0, self.rowid_base, 0)
            # 2. keys -> match
            th, tn = dtable.handles()
            streams = [D.HandleStream(th, tn)] if t.PKIsHandle else []
            streams += [D.IndexStream(di.keys.p, di.key_offsets.p, di.key_bytes, di.handles.p, di.n) for di in unique]
            if not streams:
                raise _lib.TsqError(abi.ERR_UNSUPPORTED, "REPLACE into a table without a primary key or unique index: nothing to check")
            zero = dev(n * 8)
            ctx.memset(zero, 0, n * 8)
            row_handles = allc.columns[t.pk_offset].data if t.PKIsHandle else zero  # (keys that are compared never hold the handle)
            kvs = [tablecodec.GenIndexKeys(ctx, t.ID, ix.ID, True, DeviceChunk([allc.columns[i] for i in ix.Columns], n), row_handles) for ix in uix]
            chk = D.DupChecker(ctx, streams, abi.DUP_REPLACE, None if t.PKIsHandle else th, 0 if t.PKIsHandle else tn)
            chk.push(([row_handles] if t.PKIsHandle else []) + [(k.keys, k.key_offsets, k.nbytes, k.distinct) for k in kvs], n)
            c_row, c_handle, c_ord = dev(8 * n), dev(8 * n), dev(8 * n)
            _, n_store = chk.match_replace(c_row, c_handle, c_ord)
            for k in kvs:
                k.free()
            kvs = []
            # 3. the old rows of the stored candidates: lookup -> gather -> decode
            cols = [c.col(n) for c in allc.columns]
            eq, eq2 = dev(n), dev(n)
            D.rows_equal(ctx, cols, None, cols, c_row, n, eq)
            look = tableLookupExec(ctx, dtable, self._old_columns(), True)
            if n_store:
                ords, hs = np.zeros(n, np.int64), np.zeros(n, np.int64)
                ctx.d2h(ords, c_ord)
                ctx.d2h(hs, c_handle)
                pick = np.nonzero(ords >= 0)[0]
                pos = np.full(n, -1, np.int64)
                pos[pick] = np.arange(pick.size)
                d_task, d_pos = dev(8 * pick.size), dev(8 * n)
                ctx.h2d(d_task, np.ascontiguousarray(hs[pick]))
                ctx.h2d(d_pos, pos)
                look.set_task(d_task, pick.size)
                old = look.Next()
                if old.NumRows() != pick.size:
                    raise _lib.TsqError(abi.ERR_INVALID, "REPLACE: a stored candidate's row is not in the table")
                # 4. EqualDatums against the old rows, either flag decides
                D.rows_equal(ctx, cols, None, [c.col(old.NumRows()) for c in old.columns], d_pos, n, eq2)
                _lib.check(self.lib.tsq_bytes_or(ctx.h, C.c_void_p(eq), C.c_void_p(eq2), n), ctx.h)
            cap = min(n * len(streams), tn)
            added, put = dev(n), dev(n)
            hs_out = None if t.PKIsHandle else dev(8 * n)
            r_h, r_o = ctx.alloc(8 * cap + 64), dev(8 * cap)
            try:
                res = chk.resolve(eq, self.rowid_base, added, put, hs_out, r_h, r_o, cap)
                # 5a. the deletions: record keys and ALL index keys of the removed stored rows, from their decoded old rows
                k = res.n_removed_store
                del_keys, del_kvs = None, []
                if k:
                    look.set_task(r_h, k)
                    gone = look.Next()
                    if gone.NumRows() != k:
                        raise _lib.TsqError(abi.ERR_INVALID, "REPLACE: a removed row is not in the table")
                    del_keys = ctx.alloc(k * 19 + 64)
                    free.append(del_keys)
                    _lib.check(self.lib.tsq_rowkeys_encode(ctx.h, t.ID, C.c_void_p(r_h), k, abi.COL_DEVICE, C.c_void_p(del_keys)), ctx.h)
                    for ix in self.indices:
                        del_kvs.append(tablecodec.GenIndexKeys(ctx, t.ID, ix.ID, ix.Unique, DeviceChunk([gone.columns[i] for i in ix.Columns], k), r_h))
                        kvs.append(del_kvs[-1])
                # 5b. the puts: the rows with put = 1, dense, with their handles
                m = res.n_put
                puts = None
                if m:
                    src = list(allc.columns) + ([] if t.PKIsHandle else [DeviceColumn(ctx, abi.I64, n, data=hs_out)])
                    dense = [DeviceColumn(ctx, c.tp, n, cap_bytes=c.nbytes(n) if c.var else 0) for c in src]  # (tsq_chunk_compact: sized for the input's rows)
                    try:
                        oc = (abi.Col * len(dense))(*[c.col(n) for c in dense])
                        got = C.c_int64(0)
                        _lib.check(self.lib.tsq_chunk_compact(ctx.h, (abi.Col * len(src))(*[c.col(n) for c in src]), len(src), n, C.c_void_p(put), oc, C.byref(got)), ctx.h)
                        assert got.value == m
                        if t.PKIsHandle:
                            put_handles, own = dense[t.pk_offset].data, False
                        else:
                            hc = dense.pop()
                            put_handles, own = hc.data, True
                            if hc.bitmap is not None:
                                ctx.free(hc.bitmap)
                            hc.data = hc.bitmap = None
                        puts = self._encode(DeviceChunk(dense, m), m, put_handles, own)
                    except Exception:
                        for c in dense:
                            c.free()
                        raise
            except Exception:
                ctx.free(r_h)
                raise
            kvs = []
            if del_keys:
                free.remove(del_keys)
            self.affected, self.rowid_base = res.affected, (self.rowid_base if t.PKIsHandle else res.rowid_base)
            return ReplaceBatch(ctx, k, del_keys, del_kvs, r_h, puts, res.affected, self.rowid_base, n)
        finally:
            for kv in kvs:
                kv.free()
            if look is not None:
                look.Close()
            if chk is not None:
                chk.close()
            if allc is not None:
                allc.free()
            for p in free:
                ctx.free(p)
