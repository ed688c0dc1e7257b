"""GPU parity of tsq_rows_gather (the stored rows of a lookup task, written back to back for tsq_rowcodec_decode) with numpy."""
import ctypes as C

import numpy as np
import pytest

from tinysql_amd import _abi as abi
from tinysql_amd import _lib

pytestmark = pytest.mark.gpu

GUARD = 64
PAT = 0xA7


def make_source(seed=5):
    """rows of 0, 1, 63 / 64 / 65 bytes and a few of 5 000 bytes, mixed -> (values, offsets)"""
    rng = np.random.default_rng(seed)
    lens = np.array([0, 1, 63, 64, 65, 0, 7, 8, 9, 5000, 2, 64, 5000, 0, 65, 63, 1, 5000, 31, 200] * 15, dtype=np.int64)
    rng.shuffle(lens)
    offsets = np.zeros(lens.size + 1, np.int64)
    np.cumsum(lens, out=offsets[1:])
    values = rng.integers(0, 256, int(offsets[-1]), dtype=np.uint8)
    return values, offsets


VALUES, OFFSETS = make_source()
N_SRC = OFFSETS.size - 1


def want_of(rows):
    lens = OFFSETS[rows + 1] - OFFSETS[rows]
    offs = np.zeros(rows.size + 1, np.int64)
    np.cumsum(lens, out=offs[1:])
    data = np.concatenate([VALUES[OFFSETS[r]:OFFSETS[r + 1]] for r in rows]) if rows.size else np.zeros(0, np.uint8)
    return data, offs


class Source:
    def __init__(self, ctx, values=VALUES, offsets=OFFSETS):
        self.ctx = ctx
        self.d_vals = ctx.alloc(max(values.size, 1))
        self.d_offs = ctx.alloc(offsets.nbytes)
        if values.size:
            ctx.h2d(self.d_vals, values)
        ctx.h2d(self.d_offs, offsets)
        self.n_bytes, self.n_rows = values.size, offsets.size - 1

    def call(self, rows, out_ptr, cap, offs_ptr):
        """-> (status, bytes_out)"""
        d_rows = self.ctx.alloc(max(rows.nbytes, 8))
        try:
            if rows.size:
                self.ctx.h2d(d_rows, np.ascontiguousarray(rows, dtype=np.int64))
            nb = C.c_int64(-1)
            st = self.ctx.lib.tsq_rows_gather(self.ctx.h, C.c_void_p(self.d_vals), self.n_bytes, C.c_void_p(self.d_offs), self.n_rows, C.c_void_p(d_rows), rows.size,
                                              C.c_void_p(out_ptr) if out_ptr else None, cap, C.c_void_p(offs_ptr) if offs_ptr else None, C.byref(nb))
            return st, nb.value
        finally:
            self.ctx.free(d_rows)

    def gather(self, rows, phase=0):
        """the cap_bytes = 0 query, then the real call into guarded buffers at byte phase `phase` -> (data, offsets)"""
        ctx = self.ctx
        st, need = self.call(rows, None, 0, None)
        want_data, _ = want_of(rows)
        assert need == want_data.size
        assert st == (abi.OK if need == 0 else abi.ERR_INVALID)
        if need:
            assert "too small" in _lib.last_error(ctx.h)
        out_base = ctx.alloc(need + 2 * GUARD + 16)
        offs_base = ctx.alloc((rows.size + 1 + 2 * GUARD) * 8)
        try:
            ctx.memset(out_base, PAT, need + 2 * GUARD + 16)
            ctx.memset(offs_base, PAT, (rows.size + 1 + 2 * GUARD) * 8)
            st, got = self.call(rows, out_base + GUARD + phase, need, offs_base + GUARD * 8)
            _lib.check(st, ctx.h)
            assert got == need
            out = np.zeros(need + 2 * GUARD + 16, np.uint8)
            offs = np.zeros((rows.size + 1 + 2 * GUARD) * 8, np.uint8)
            ctx.d2h(out, out_base)
            ctx.d2h(offs, offs_base)
            lo = GUARD + phase
            assert (out[:lo] == PAT).all() and (out[lo + need:] == PAT).all(), "bytes outside the output were written"
            assert (offs[:GUARD * 8] == PAT).all() and (offs[(GUARD + rows.size + 1) * 8:] == PAT).all(), "offsets outside the output were written"
            return out[lo:lo + need].copy(), offs[GUARD * 8:(GUARD + rows.size + 1) * 8].view(np.int64).copy()
        finally:
            ctx.free(out_base)
            ctx.free(offs_base)

    def close(self):
        self.ctx.free(self.d_vals)
        self.ctx.free(self.d_offs)


@pytest.fixture(scope="module")
def src(ctx):
    s = Source(ctx)
    yield s
    s.close()


def row_lists():
    rng = np.random.default_rng(9)
    return {
        "all": np.arange(N_SRC, dtype=np.int64),
        "reversed": np.arange(N_SRC, dtype=np.int64)[::-1].copy(),
        "repeated": np.repeat(rng.integers(0, N_SRC, 40), 3).astype(np.int64),
        "random_65": rng.integers(0, N_SRC, 65).astype(np.int64),
        "one": np.array([int(np.argmax(np.diff(OFFSETS) == 5000))], dtype=np.int64),
        "only_empty_rows": np.flatnonzero(np.diff(OFFSETS) == 0).astype(np.int64),
        "empty": np.zeros(0, np.int64),
    }


ROW_LISTS = row_lists()


@pytest.mark.parametrize("wave_copy", [0, 8, None, 1 << 20])  # never, 8, the default, above every row length
@pytest.mark.parametrize("name", list(ROW_LISTS))
def test_gather_equals_numpy(ctx, src, wave_copy, name):
    if wave_copy is not None:
        ctx.set_knob(abi.KNOB_GATHER_WAVE_COPY, wave_copy)
    rows = ROW_LISTS[name]
    data, offs = src.gather(rows)
    want_data, want_offs = want_of(rows)
    assert (offs == want_offs).all()
    assert data.tobytes() == want_data.tobytes()


@pytest.mark.parametrize("wave_copy", [0, 8, None])
@pytest.mark.parametrize("phase", [0, 1, 7, 8, 15])
def test_output_pointer_phase(ctx, src, wave_copy, phase):
    if wave_copy is not None:
        ctx.set_knob(abi.KNOB_GATHER_WAVE_COPY, wave_copy)
    rows = ROW_LISTS["random_65"]
    data, offs = src.gather(rows, phase)
    want_data, want_offs = want_of(rows)
    assert (offs == want_offs).all() and data.tobytes() == want_data.tobytes()


def test_more_rows_than_one_launch_step(ctx, src):
    rows = np.random.default_rng(2).integers(0, N_SRC, 20001).astype(np.int64)
    rows = rows[np.diff(OFFSETS)[rows] < 100]  # (keeps the output small)
    for wc in (8, 1 << 20):
        ctx.set_knob(abi.KNOB_GATHER_WAVE_COPY, wc)
        data, offs = src.gather(rows)
        want_data, want_offs = want_of(rows)
        assert (offs == want_offs).all() and data.tobytes() == want_data.tobytes()


def test_errors_write_nothing(ctx, src):
    good = ROW_LISTS["random_65"]
    need = want_of(good)[0].size
    out = ctx.alloc(need + 64)
    offs = ctx.alloc((good.size + 1) * 8)
    try:
        for bad_value in (N_SRC, -1, 1 << 40, -(1 << 62)):
            rows = good.copy()
            rows[33] = bad_value
            ctx.memset(out, PAT, need + 64)
            ctx.memset(offs, PAT, (good.size + 1) * 8)
            st, nb = src.call(rows, out, need + 64, offs)
            assert st == abi.ERR_INVALID and "row index out of range" in _lib.last_error(ctx.h), bad_value
            h_out, h_offs = np.zeros(need + 64, np.uint8), np.zeros((good.size + 1) * 8, np.uint8)
            ctx.d2h(h_out, out)
            ctx.d2h(h_offs, offs)
            assert (h_out == PAT).all() and (h_offs == PAT).all()
        # a too small buffer: the size comes back, nothing is written
        ctx.memset(out, PAT, need + 64)
        st, nb = src.call(good, out, need - 1, offs)
        assert st == abi.ERR_INVALID and nb == need
        h_out = np.zeros(need + 64, np.uint8)
        ctx.d2h(h_out, out)
        assert (h_out == PAT).all()
        st, nb = src.call(good, out, need, offs)
        assert st == abi.OK and nb == need
        # argument contract
        lib = ctx.lib
        nbv = C.c_int64(0)
        assert lib.tsq_rows_gather(ctx.h, C.c_void_p(src.d_vals), src.n_bytes, C.c_void_p(src.d_offs), src.n_rows, None, 3, C.c_void_p(out), 10, C.c_void_p(offs), C.byref(nbv)) == abi.ERR_INVALID
        assert lib.tsq_rows_gather(ctx.h, C.c_void_p(src.d_vals), src.n_bytes, C.c_void_p(src.d_offs), src.n_rows, C.c_void_p(offs), -1, C.c_void_p(out), 10, C.c_void_p(offs), C.byref(nbv)) == abi.ERR_INVALID
        assert lib.tsq_rows_gather(ctx.h, C.c_void_p(src.d_vals), src.n_bytes, C.c_void_p(src.d_offs), src.n_rows, C.c_void_p(offs), 1, None, 10, C.c_void_p(offs), C.byref(nbv)) == abi.ERR_INVALID
        assert lib.tsq_rows_gather(ctx.h, C.c_void_p(src.d_vals), src.n_bytes, C.c_void_p(src.d_offs), src.n_rows, C.c_void_p(offs), 1, C.c_void_p(out), 10, C.c_void_p(offs), None) == abi.ERR_INVALID
    finally:
        ctx.free(out)
        ctx.free(offs)


def test_decreasing_offset_pair_is_refused(ctx):
    offsets = np.array([0, 10, 30, 20, 40], dtype=np.int64)  # row 2 = [30, 20)
    values = np.arange(40, dtype=np.uint8)
    s = Source(ctx, values, offsets)
    out = ctx.alloc(256)
    offs = ctx.alloc(64)
    try:
        st, nb = s.call(np.array([0, 1], dtype=np.int64), out, 256, offs)
        assert st == abi.OK and nb == 30
        st, nb = s.call(np.array([0, 2, 1], dtype=np.int64), out, 256, offs)
        assert st == abi.ERR_INVALID and "offsets must not decrease" in _lib.last_error(ctx.h)
        # an offset pair that leaves the values is refused as well: nothing is read beyond n_bytes
        s2 = Source(ctx, values, np.array([0, 10, 4000], dtype=np.int64))
        try:
            st, nb = s2.call(np.array([1], dtype=np.int64), out, 256, offs)
            assert st == abi.ERR_INVALID
        finally:
            s2.close()
    finally:
        s.close()
        ctx.free(out)
        ctx.free(offs)
