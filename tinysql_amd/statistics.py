"""The statistics an ANALYZE TABLE collects, over libtsq — the harness mirror of package statistics as far as the storage side fills
it (store/mockstore/mocktikv/analyze.go:34-219): FMSketch (fmsketch.go), CMSketch (cmsketch.go), SampleCollector (sample.go:74-177) and
the Histogram a SortedBuilder leaves (builder.go:24-94, histogram.go:43-72).

The objects are plain host values filled from the device handles: `AnalyzeCollector` (tsq_analyze_*) is SampleBuilder.CollectColumnStats
without its PK builder, `SortedBuilder` (tsq_sorted_hist_*) is the builder of the PK / index histogram.  The merges are what
AnalyzeColumnsExec.buildStats does with the responses of several regions, on the host: they touch a few thousand values.
Semantics (the canonical FM sketch, the CM counter formula, the deterministic sampler): DESIGN.md "ANALYZE"."""
import ctypes as C

import numpy as np

from . import _abi as abi
from . import _lib
from .chunk import Column, StrColumn, make_cols

M64 = (1 << 64) - 1


def _splitmix64(x):
    x = (x + 0x9E3779B97F4A7C15) & M64
    z = x
    z = ((z ^ (z >> 30)) * 0xBF58476D1CE4E5B9) & M64
    z = ((z ^ (z >> 27)) * 0x94D049BB133111EB) & M64
    return z ^ (z >> 31)


class FMSketch:
    """statistics.FMSketch in canonical form: mask = 2^k - 1 for the smallest k at which the distinct hashes with h & mask == 0
    number at most maxSize; hashset = those hashes."""

    def __init__(self, maxSize, mask=0, hashset=()):
        self.maxSize, self.mask, self.hashset = int(maxSize), int(mask), set(int(h) for h in hashset)

    def NDV(self):  # fmsketch.go:44-47
        return (self.mask + 1) * len(self.hashset)

    def mergeFMSketch(self, rs):
        """fmsketch.go:96-106, canonical: both sets are complete at the larger mask, so the result is the sketch of the union of the inputs"""
        mask = max(self.mask, rs.mask)
        hs = {h for h in self.hashset | rs.hashset if h & mask == 0}
        while len(hs) > self.maxSize:
            mask = mask * 2 + 1
            hs = {h for h in hs if h & mask == 0}
        self.mask, self.hashset = mask, hs

    def __eq__(self, o):
        return isinstance(o, FMSketch) and (self.mask, self.hashset) == (o.mask, o.hashset)


class CMSketch:
    """statistics.CMSketch: depth x width uint32 counters and the number of inserted values."""

    def __init__(self, depth, width, count=0, table=None):
        self.depth, self.width, self.count = int(depth), int(width), int(count)
        self.table = np.zeros((self.depth, self.width), np.uint32) if table is None else np.asarray(table, np.uint32).reshape(self.depth, self.width).copy()

    def MergeCMSketch(self, rc):  # cmsketch.go:69-83
        if (self.depth, self.width) != (rc.depth, rc.width):
            raise ValueError("Dimensions of Count-Min Sketch should be the same")
        self.count += rc.count
        self.table = self.table + rc.table  # (uint32 wrap-around, as the reference's counters)
        return None

    def queryHashValue(self, h1, h2):
        """the estimate for a value with the murmur3 pair (h1, h2): the smallest of its counters"""
        return int(min(self.table[i, ((h1 + h2 * i) & M64) % self.width] for i in range(self.depth)))

    def __eq__(self, o):
        return isinstance(o, CMSketch) and self.count == o.count and self.table.shape == o.table.shape and bool((self.table == o.table).all())


class SampleCollector:
    """statistics.SampleCollector: Samples are the cell values in row order (None never occurs: a NULL is not sampled), Ordinals
    their row numbers among the pushed rows."""

    def __init__(self, MaxSampleSize, FMSketch=None, CMSketch=None):
        self.Samples, self.Ordinals = [], []
        self.seenValues = 0
        self.NullCount = self.Count = self.TotalSize = 0
        self.MaxSampleSize, self.FMSketch, self.CMSketch = int(MaxSampleSize), FMSketch, CMSketch

    def _collect_merged(self, v):
        """collect of a merger (sample.go:159-176).  The reference draws from Go's global math/rand; here the draw is a function of
        seenValues, so a merge is repeatable (parity unpinned, like the sampler itself)."""
        self.seenValues += 1
        if len(self.Samples) < self.MaxSampleSize:
            self.Samples.append(v)
            return
        r = _splitmix64(self.seenValues)
        if r % self.seenValues < self.MaxSampleSize:
            idx = _splitmix64(r) % self.MaxSampleSize
            del self.Samples[idx]  # delete and append keeps the order of the elements
            self.Samples.append(v)

    def MergeSampleCollector(self, rc):  # sample.go:88-101
        self.NullCount += rc.NullCount
        self.Count += rc.Count
        self.TotalSize += rc.TotalSize
        self.FMSketch.mergeFMSketch(rc.FMSketch)
        if rc.CMSketch is not None:
            self.CMSketch.MergeCMSketch(rc.CMSketch)
        self.Ordinals = []  # (row numbers of different regions do not compare)
        for v in rc.Samples:
            self._collect_merged(v)


class Bucket:
    def __init__(self, Count, Repeat):
        self.Count, self.Repeat = int(Count), int(Repeat)

    def __eq__(self, o):
        return (self.Count, self.Repeat) == (o.Count, o.Repeat)

    def __repr__(self):
        return "Bucket(%d, %d)" % (self.Count, self.Repeat)


class Histogram:
    """statistics.Histogram of a SortedBuilder: cumulative counts, the repeats of every upper bound, the bounds as values (and as row
    numbers of the sorted input)."""

    def __init__(self, NDV=0, Buckets=(), lower=(), upper=(), lower_rows=(), upper_rows=()):
        self.NDV, self.Buckets = int(NDV), list(Buckets)
        self.lower, self.upper, self.lower_rows, self.upper_rows = list(lower), list(upper), list(lower_rows), list(upper_rows)

    def Len(self):
        return len(self.Buckets)

    def TotalRowCount(self):  # histogram.go:291-296
        return self.Buckets[-1].Count if self.Buckets else 0

    def GetLower(self, i):
        return self.lower[i]

    def GetUpper(self, i):
        return self.upper[i]


def _push_cols(chunk, keep):
    """a host Chunk / list of columns, or a gpu_pipeline.DeviceChunk -> (tsq_col array, rows)"""
    if hasattr(chunk, "cols"):
        return chunk.cols(), chunk.NumRows()
    columns = chunk.columns if hasattr(chunk, "columns") else list(chunk)
    return make_cols(columns, keep), (len(columns[0]) if columns else 0)


class AnalyzeCollector:
    """tsq_analyze_*: SampleBuilder.CollectColumnStats over pushed chunks.  types: abi.I64 .. abi.BYTES per column; col_flags:
    abi.ENC_COMPARABLE | abi.AN_RAW per column; wrap_bytes: the FM sketch hashes the bytes datum of the encoded value, what the
    storage side of an ANALYZE does (analyze.go:236)."""

    def __init__(self, ctx, types, MaxSampleSize, MaxFMSketchSize, CMSketchDepth=0, CMSketchWidth=0, col_flags=None, wrap_bytes=False, seed=0):
        self.ctx, self.lib, self.types = ctx, ctx.lib, list(types)
        cfg = abi.AnalyzeCfg()
        cfg.n_cols = len(self.types)
        for i, t in enumerate(self.types):
            cfg.col_types[i] = t
            cfg.col_flags[i] = col_flags[i] if col_flags else 0
        cfg.max_sample_size, cfg.max_fm_size = MaxSampleSize, MaxFMSketchSize
        cfg.cm_depth, cfg.cm_width = CMSketchDepth, CMSketchWidth
        cfg.flags = abi.AN_WRAP_BYTES if wrap_bytes else 0
        cfg.sample_seed = seed & M64
        self.cfg = cfg
        self.h = C.c_void_p()
        _lib.check(self.lib.tsq_analyze_create(ctx.h, C.byref(cfg), C.byref(self.h)), ctx.h)

    def push(self, chunk):
        keep = []
        cols, n = _push_cols(chunk, keep)
        _lib.check(self.lib.tsq_analyze_push(self.h, cols, len(self.types), n), self.h)

    def cancel(self):
        self.lib.tsq_analyze_cancel(self.h)

    def finish(self):
        """-> one SampleCollector per column"""
        _lib.check(self.lib.tsq_analyze_finish(self.h), self.h)
        return [self._column(c) for c in range(len(self.types))]

    def _column(self, c):
        lib, h, cfg = self.lib, self.h, self.cfg
        nulls, cnt, size, fsz, ccnt, ns = (C.c_int64(0) for _ in range(6))
        mask = C.c_uint64(0)
        _lib.check(lib.tsq_analyze_column(h, c, C.byref(nulls), C.byref(cnt), C.byref(size), C.byref(mask), C.byref(fsz), C.byref(ccnt), C.byref(ns)), h)
        hashes = np.zeros(max(fsz.value, 1), np.uint64)
        _lib.check(lib.tsq_analyze_fm(h, c, hashes.ctypes.data_as(C.c_void_p), fsz.value), h)
        cm = None
        if cfg.cm_depth:
            tab = np.zeros(cfg.cm_depth * cfg.cm_width, np.uint32)
            _lib.check(lib.tsq_analyze_cm(h, c, tab.ctypes.data_as(C.c_void_p)), h)
            cm = CMSketch(cfg.cm_depth, cfg.cm_width, ccnt.value, tab)
        sc = SampleCollector(cfg.max_sample_size, FMSketch(cfg.max_fm_size, mask.value, hashes[:fsz.value].tolist()), cm)
        sc.NullCount, sc.Count, sc.TotalSize = nulls.value, cnt.value, size.value
        n, nbytes = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.tsq_analyze_samples_peek(h, c, C.byref(n), C.byref(nbytes)), h)
        tp = self.types[c]
        out = abi.Col()
        ords = np.zeros(max(n.value, 1), np.int64)
        out.length, out.type, out.flags = n.value, tp, 0
        if tp == abi.BYTES:
            data, offs = np.zeros(nbytes.value + 8, np.uint8), np.zeros(n.value + 1, np.int64)
            out.data, out.offsets, out.elem_size = data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), -1
        else:
            data = np.zeros(max(n.value, 1), {abi.I64: np.int64, abi.U64: np.uint64, abi.F32: np.float32, abi.F64: np.float64}[tp])
            out.data, out.elem_size = data.ctypes.data_as(C.c_void_p), data.itemsize
        _lib.check(lib.tsq_analyze_samples(h, c, C.byref(out), ords.ctypes.data_as(C.c_void_p), n.value), h)
        if tp == abi.BYTES:
            raw = data.tobytes()
            sc.Samples = [raw[offs[i]:offs[i + 1]] for i in range(n.value)]
        else:
            sc.Samples = data[:n.value].tolist()
        sc.Ordinals = ords[:n.value].tolist()
        sc.seenValues = sc.Count
        return sc

    def stats(self):
        rows, ms = C.c_int64(0), C.c_double(0)
        _lib.check(self.lib.tsq_analyze_stats(self.h, C.byref(rows), C.byref(ms)), self.h)
        return {"rows": rows.value, "kernel_ms": ms.value}

    def close(self):
        if self.h:
            self.lib.tsq_analyze_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


class SortedBuilder:
    """tsq_sorted_hist_*: statistics.SortedBuilder over a pushed, sorted column (abi.I64 | abi.U64 | abi.BYTES)."""

    def __init__(self, ctx, tp, numBuckets):
        self.ctx, self.lib, self.tp = ctx, ctx.lib, tp
        self.h = C.c_void_p()
        _lib.check(self.lib.tsq_sorted_hist_create(ctx.h, tp, numBuckets, C.byref(self.h)), ctx.h)
        self.Count = 0

    def push(self, column, nrows=None):
        """column: a host Column / StrColumn, or a device column (gpu_pipeline.DeviceColumn) with nrows"""
        keep = []
        if nrows is None:
            col, nrows = column.as_col(keep), len(column)
        else:
            col = column.col(nrows)
        _lib.check(self.lib.tsq_sorted_hist_push(self.h, C.byref(col), nrows), self.h)

    def Hist(self):
        lib, h = self.lib, self.h
        _lib.check(lib.tsq_sorted_hist_finish(h), h)
        nb, lb, ub = C.c_int64(0), C.c_int64(0), C.c_int64(0)
        _lib.check(lib.tsq_sorted_hist_peek(h, C.byref(nb), C.byref(lb), C.byref(ub)), h)
        n = nb.value
        arrs = [np.zeros(max(n, 1), np.int64) for _ in range(4)]
        bounds, bufs = [], []
        for nbytes in (lb.value, ub.value):
            c = abi.Col()
            c.length, c.type, c.flags = n, self.tp, 0
            if self.tp == abi.BYTES:
                data, offs = np.zeros(nbytes + 8, np.uint8), np.zeros(n + 1, np.int64)
                c.data, c.offsets, c.elem_size = data.ctypes.data_as(C.c_void_p), offs.ctypes.data_as(C.c_void_p), -1
                bufs.append((data, offs))
            else:
                data = np.zeros(max(n, 1), np.uint64 if self.tp == abi.U64 else np.int64)
                c.data, c.elem_size = data.ctypes.data_as(C.c_void_p), 8
                bufs.append((data, None))
            bounds.append(c)
        cnt, ndv = C.c_int64(0), C.c_int64(0)
        _lib.check(lib.tsq_sorted_hist_result(h, C.byref(nb), C.byref(cnt), C.byref(ndv), *[a.ctypes.data_as(C.c_void_p) for a in arrs],
                                              C.byref(bounds[0]), C.byref(bounds[1])), h)
        self.Count = cnt.value
        vals = []
        for data, offs in bufs:
            if offs is None:
                vals.append(data[:n].tolist())
            else:
                raw = data.tobytes()
                vals.append([raw[offs[i]:offs[i + 1]] for i in range(n)])
        return Histogram(ndv.value, [Bucket(arrs[0][i], arrs[1][i]) for i in range(n)], vals[0], vals[1], arrs[2][:n].tolist(), arrs[3][:n].tolist())

    def stats(self):
        rows, steps, a, b = C.c_int64(0), C.c_int64(0), C.c_double(0), C.c_double(0)
        _lib.check(self.lib.tsq_sorted_hist_stats(self.h, C.byref(rows), C.byref(a), C.byref(b), C.byref(steps)), self.h)
        return {"rows": rows.value, "scan_ms": a.value, "walk_ms": b.value, "steps": steps.value}

    def close(self):
        if self.h:
            self.lib.tsq_sorted_hist_destroy(self.h)
            self.h = None

    def __enter__(self):
        return self

    def __exit__(self, *a):
        self.close()


__all__ = ["FMSketch", "CMSketch", "SampleCollector", "Bucket", "Histogram", "AnalyzeCollector", "SortedBuilder", "Column", "StrColumn"]
