"""GPU parity of tsq_dupcheck_* (INSERT .. SELECT's duplicate-key check, REPLACE .. SELECT's row logic) with the SEQUENTIAL model of
tests/dupcheck_ref.py: flags, handles, counts, the removed stored rows and the final table are compared exactly; the candidates of the
equality test with the parallel form of tests/dupcheck_form.py (which tests/test_dupcheck_cpu.py holds to the model)."""
import numpy as np
import pytest

from tests import dupcheck_gpu_helpers as G
from tests import dupcheck_ref as R
from tinysql_amd import _abi as abi
from tinysql_amd import _lib
from tinysql_amd import dupcheck as D

pytestmark = pytest.mark.gpu

I64_MIN, I64_MAX = -(1 << 63), (1 << 63) - 1
ROWS = [0, 1, 63, 64, 65, 1023, 1024, 1025, 4097]
STORES = [0, 1, 15, 16, 17, 4097]

PK = R.TableShape([abi.I64, abi.I64], 0)
PK_UV = R.TableShape([abi.I64, abi.I64], 0, [[(1, None)]])
CHAIN = R.TableShape([abi.I64, abi.I64, abi.I64, abi.I64], 0, [[(1, None)], [(2, None)]])


def store_rows(shape, m, step=3):
    """m consistent stored rows with handles 0, step, 2 * step, ...; every column of row k = its handle (so unique everywhere)"""
    return [(k * step, (k * step,) * len(shape.col_types)) for k in range(m)]


# ---------------------------------------------------------------- statement sizes x collision patterns
def pattern_rows(pattern, n):
    if pattern == "identical":  # one content: the first is added, every later one is unchanged
        return PK_UV, [(4, 7)] * n
    if pattern == "distinct":  # nothing collides inside the statement; a third of the rows meet a stored row, half of those unchanged
        return PK_UV, [(r, r if r % 2 else r + 100000) for r in range(n)]
    if pattern == "alternating":  # A B A B with one key: nothing is unchanged, every row but the last is removed again
        return PK, [(1, 10 + (r & 1)) for r in range(n)]
    # chain: row r collides with row r + 1 on stream r % 3
    return CHAIN, [(r - 1 if r % 3 == 1 else r, r - 1 if r % 3 == 2 else r, r - 1 if r % 3 == 0 and r else r, r) for r in range(n)]


@pytest.mark.parametrize("pattern", ["identical", "distinct", "alternating", "chain"])
@pytest.mark.parametrize("n", ROWS)
def test_replace_statement_sizes_and_collision_patterns(ctx, n, pattern):
    shape, rows = pattern_rows(pattern, n)
    got, want = G.check_replace(ctx, shape, store_rows(shape, 17), rows)
    if pattern == "identical" and n > 1:
        assert got["added"].count(True) == 1
    if pattern == "alternating" and n > 1:
        assert got["put"].count(True) == 1 and got["n_removed_batch"] == n - 1
    if pattern == "chain" and n > 3:
        assert got["n_removed_batch"] > n // 2


# ---------------------------------------------------------------- store sizes, the ends of the store, extreme handles
@pytest.mark.parametrize("m", STORES)
@pytest.mark.parametrize("mode", ["replace", "insert"])
def test_store_sizes_first_last_below_above_and_extreme_handles(ctx, m, mode):
    stored = store_rows(PK_UV, m)
    if m >= 2:  # INT64_MIN / INT64_MAX are ordinary handles
        stored[0] = (I64_MIN, (I64_MIN, -5))
        stored[-1] = (I64_MAX, (I64_MAX, 3 * m + 5))
    hs = [h for h, _ in stored]
    vs = [r[1] for _, r in stored]
    rows = []
    if m:
        rows += [(hs[0], 777001), (hs[-1], 777002)]  # the first and the last stored handle
        rows += [(900001, min(vs)), (900002, max(vs))]  # the first and the last stored index key
        rows += [(900003, min(vs) - 1), (900004, max(vs) + 1)]  # below the first, above the last index key
        rows += [(hs[len(hs) // 2], vs[len(vs) // 2])]  # an unchanged row when it is the stored one
    rows += [(I64_MIN + 1, -99), (I64_MAX - 1, 99), (1, 1), (2, 888), (I64_MIN, 5), (I64_MAX, 6)]
    rows += [(3 * k + 1, 3 * k + 1) for k in range(60)]  # between the stored keys
    if mode == "replace":
        G.check_replace(ctx, PK_UV, stored, rows)
    else:
        for cut in (len(rows), 7, 4, 2):  # the statement shortened so that other rows are the first to fail
            G.check_insert(ctx, PK_UV, stored, rows[len(rows) - cut:])


# ---------------------------------------------------------------- string index keys
def words():
    """cells of 0..70 bytes sharing prefixes: pairs that differ only in their last byte and only in length"""
    base = bytes(range(33, 33 + 70))
    out = [b""]
    for n in range(1, 71):
        out += [base[:n], base[:n - 1] + b"~", base[:n - 1] + b"\0"]
    return out


def test_string_keys_prefix_index_and_null_cells_without_a_pk_handle(ctx):
    # (s VARCHAR UNIQUE, t VARCHAR with UNIQUE (t(3)), (a, u) UNIQUE with NULLs, payload DOUBLE); the handle is _tidb_rowid
    shape = R.TableShape([abi.BYTES, abi.BYTES, abi.I64, abi.BYTES, abi.F64], None, [[(0, None)], [(1, 3)], [(2, None), (3, None)]])
    w = words()
    rng = np.random.default_rng(5)
    mk = lambda i, j, a, u, f: (w[i % len(w)], b"p%02d-tail%d" % (j % 50, j), a, u, f)
    store = R.Store(shape)
    res = R.replace_stmt(shape, store, [mk(3 * k, k, k % 9, b"u%d" % (k % 4), 0.0) for k in range(40)], 0)
    stored = sorted(store.table().items())
    rows = []
    for r in range(300):
        a = None if r % 7 == 0 else int(rng.integers(0, 9))
        u = None if r % 11 == 0 else b"u%d" % int(rng.integers(0, 4))
        rows.append(mk(int(rng.integers(0, len(w))), int(rng.integers(0, 400)), a, u, [0.0, -0.0, float("nan")][r % 3]))
        if r % 5 == 0 and stored:  # a stored row again, cell for cell: unchanged, in the middle of the rowid scan
            rows.append(stored[int(rng.integers(0, len(stored)))][1])
        if r % 9 == 0:  # the previous row again
            rows.append(rows[-1])
    got, want = G.check_replace(ctx, shape, stored, rows, rowid_base=res["rowid_base"])
    assert 0 < got["added"].count(False) and got["n_removed_batch"] > 0 and got["removed_store"]
    G.check_insert(ctx, shape, stored, rows, rowid_base=res["rowid_base"])
    # NULL in either column of (a, u): not distinct, matches nothing — neither the stored (None, u1) / (3, None) rows nor each other
    nulls = [mk(2, 40, None, b"u1", 1.0), mk(5, 41, None, b"u1", 1.0), mk(8, 42, 3, None, 1.0), mk(11, 43, 3, None, 1.0)]
    more = sorted(stored + [(res["rowid_base"] + 1 + k, r) for k, r in enumerate([mk(14, 44, None, b"u1", 1.0), mk(17, 45, 3, None, 1.0)])])
    assert G.check_insert(ctx, shape, more, nulls, rowid_base=res["rowid_base"] + 2) is None
    got, _ = G.check_replace(ctx, shape, more, nulls, rowid_base=res["rowid_base"] + 2)
    assert got["added"] == [True] * 4 and got["removed_store"] == []


# ---------------------------------------------------------------- 1, 2 and 8 streams
@pytest.mark.parametrize("n_streams", [1, 2, 8])
@pytest.mark.parametrize("with_pk", [True, False])
def test_stream_counts(ctx, n_streams, with_pk):
    n_idx = n_streams - (1 if with_pk else 0)
    shape = R.TableShape([abi.I64] * 9, 0 if with_pk else None, [[(c, None)] for c in range(1, 1 + n_idx)])
    rng = np.random.default_rng(n_streams)
    store = R.Store(shape)
    res = R.replace_stmt(shape, store, [tuple(int(x) for x in rng.integers(0, 40, 9)) for _ in range(30)], 0)
    stored = sorted(store.table().items())
    rows = [tuple(int(x) for x in rng.integers(0, 40, 9)) for _ in range(200)] + [r for _, r in stored[:5]]
    G.check_replace(ctx, shape, stored, rows, rowid_base=res["rowid_base"])
    G.check_insert(ctx, shape, stored, rows, rowid_base=res["rowid_base"])


def test_rowid_scan_with_unchanged_rows_in_the_middle(ctx):
    shape = R.TableShape([abi.I64, abi.I64], None, [[(0, None)]])
    stored = [(10 + k, (k, k)) for k in range(100)]
    rows = [(k, k if k % 3 else -k) for k in range(50, 150)]  # two thirds of the first fifty are the stored rows again
    got, want = G.check_replace(ctx, shape, stored, rows, rowid_base=500)
    assert got["added"].count(False) == 33 and got["rowid_base"] == 500 + 67
    assert [h for h in got["handles"] if h is not None] == list(range(501, 568))


# ---------------------------------------------------------------- INSERT mode
def test_insert_first_error_among_several_rows_and_streams(ctx):
    stored = store_rows(CHAIN, 20)
    ok = [(1000 + r, 1000 + r, 1000 + r, r) for r in range(3000)]
    assert G.check_insert(ctx, CHAIN, stored, ok) is None
    rows = list(ok)
    rows[2900] = (6, 9, 12, 0)  # fails on all three streams: the handle's stream is the error's
    rows[2500] = (5000, 5001, 12, 0)  # an earlier row that fails on the last stream only
    rows[2700] = (5002, 9, 5003, 0)
    got = G.check_insert(ctx, CHAIN, stored, rows)
    assert (got.row, got.stream, got.from_store, got.dup_handle) == (2500, 2, True, 12)
    got = G.check_insert(ctx, CHAIN, stored, rows[2501:])
    assert (got.row, got.stream, got.dup_handle) == (199, 1, 9)
    got = G.check_insert(ctx, CHAIN, stored, rows[2701:])
    assert (got.row, got.stream, got.dup_handle) == (199, 0, 6)


def test_insert_stored_and_in_batch_conflict_on_the_same_key(ctx):
    stored = store_rows(PK_UV, 5)  # handles and values 0, 3, 6, 9, 12
    # row 1 repeats row 0's index key, which is stored too: row 0 fails first, on the store
    got = G.check_insert(ctx, PK_UV, stored, [(100, 6), (101, 6)])
    assert (got.row, got.stream, got.from_store, got.dup_handle) == (0, 1, True, 6)
    # in the batch alone: the conflict is with the FIRST row of the key's group
    got = G.check_insert(ctx, PK_UV, stored, [(100, 7), (101, 8), (102, 7), (103, 7)])
    assert (got.row, got.stream, got.from_store, got.dup_row) == (2, 1, False, 0)
    got = G.check_insert(ctx, PK_UV, stored, [(100, 7), (100, 8)])
    assert (got.row, got.stream, got.from_store, got.dup_row) == (1, 0, False, 0)
    # one row meets the store on a later stream while an earlier stream has an in-batch conflict: stream order decides
    got = G.check_insert(ctx, PK_UV, stored, [(100, 7), (100, 9)])
    assert (got.row, got.stream, got.from_store) == (1, 0, False)


@pytest.mark.parametrize("n", [1, 65, 1025, 4097])
def test_insert_sizes_with_the_only_conflict_in_the_last_row(ctx, n):
    stored = store_rows(PK_UV, 17)
    rows = [(1000 + r, 1000 + r) for r in range(n - 1)] + [(5, 9)]
    got = G.check_insert(ctx, PK_UV, stored, rows)
    assert (got.row, got.stream, got.dup_handle) == (n - 1, 1, 9)
    rows[-1] = (5, 1000) if n > 1 else (3, 5)
    got = G.check_insert(ctx, PK_UV, stored, rows)
    assert (got.row, got.stream) == (n - 1, 1 if n > 1 else 0)


# ---------------------------------------------------------------- pushes
@pytest.mark.parametrize("split", [1, 64, 1000])
def test_split_pushes_give_the_answer_of_one_push(ctx, split):
    shape = R.TableShape([abi.I64, abi.I64, abi.BYTES], 0, [[(1, None)], [(2, None)]])
    rng = np.random.default_rng(9)
    n = 300 if split == 1 else 2100
    rows = [(int(rng.integers(0, 500)), int(rng.integers(0, 500)), b"w%d" % int(rng.integers(0, 500))) for _ in range(n)]
    stored = [(k, (k, k, b"w%d" % k)) for k in range(0, 500, 7)]
    st = G.Statement(ctx, shape, stored, rows)
    try:
        one, cut = st.replace(), st.replace(splits=split)
        assert cut["stats"]["pushes"] == -(-n // split) and one["stats"]["pushes"] == 1
        for k in ("cand", "equal", "added", "put", "handles", "removed_store", "n_removed_batch", "affected"):
            assert one[k] == cut[k], k
        a, b = st.insert(), st.insert(splits=split)
        assert (a.row, a.stream, a.from_store, a.dup_handle, a.dup_row) == (b.row, b.stream, b.from_store, b.dup_handle, b.dup_row)
    finally:
        st.free()
    G.check_replace(ctx, shape, stored, rows, splits=split)


def test_reset_takes_the_next_statement_against_the_same_store(ctx):
    shape = R.TableShape([abi.I64, abi.BYTES], 0, [[(1, None)]])
    stored = [(k, (k, b"w%d" % k)) for k in range(0, 300, 3)]
    a = G.Statement(ctx, shape, stored, [(1000 + r, b"n%d" % r) for r in range(500)] + [(7, b"w9")])
    b = G.Statement(ctx, shape, stored, [(2000, b"x"), (2001, b"w30"), (6, b"y")])
    c = G.Statement(ctx, shape, stored, [(3000 + r, b"m%d" % r) for r in range(70)])
    chk = a.checker(abi.DUP_INSERT)
    try:
        e = chk.match_insert()
        assert (e.row, e.stream, e.dup_handle) == (500, 1, 9)
        for st, want in ((b, (1, 1, 30)), (c, None), (a, (500, 1, 9))):  # a shorter statement, a clean one, the first again
            chk.reset()
            st.push_into(chk, 64)
            e = chk.match_insert()
            assert (None if e is None else (e.row, e.stream, e.dup_handle)) == want and chk.stats()["rows"] == st.n
    finally:
        chk.close()
        for st in (a, b, c):
            st.free()


# ---------------------------------------------------------------- random statements
def test_random_statements_equal_the_model(ctx):
    from tests.test_dupcheck_cpu import random_rows, random_shape, random_store
    rng = np.random.default_rng(77)
    for it in range(150):
        shape = random_shape(rng)
        if shape.n_streams() == 0:
            continue
        dom = int(rng.integers(2, 13))
        stored, base = random_store(rng, shape, dom)
        rows = random_rows(rng, int(rng.integers(0, 40)), dom, [r for _, r in stored])
        G.check_replace(ctx, shape, stored, rows, rowid_base=base)
        G.check_insert(ctx, shape, stored, rows, rowid_base=base)


# ---------------------------------------------------------------- refusals
def test_refusals(ctx):
    st = G.Statement(ctx, PK_UV, store_rows(PK_UV, 5), [(1, 1), (3, 4)])
    try:
        hs, ix = st.streams
        with pytest.raises(_lib.TsqError, match="more than TSQ_DUP_MAX_STREAMS") as e:
            D.DupChecker(ctx, [hs] + [ix] * 8, abi.DUP_REPLACE)
        assert e.value.status == abi.ERR_INVALID
        with pytest.raises(_lib.TsqError, match="no stream"):
            D.DupChecker(ctx, [], abi.DUP_INSERT)
        with pytest.raises(_lib.TsqError, match="two HANDLE streams"):
            D.DupChecker(ctx, [hs, hs], abi.DUP_INSERT)
        # unsorted store: index keys, then table handles
        ks, _ = R.index_keys(PK_UV, 0, [(0, 9), (0, 3)])
        raw, offs = st.up(np.frombuffer(ks[0] + ks[1], np.uint8)), st.up(np.array([0, len(ks[0]), len(ks[0]) + len(ks[1])], np.int64))
        two = st.up(np.array([9, 3], np.int64))
        with pytest.raises(_lib.TsqError, match="index keys not ascending") as e:
            D.DupChecker(ctx, [hs, D.IndexStream(raw.p, offs.p, len(ks[0]) + len(ks[1]), two.p, 2)], abi.DUP_INSERT)
        assert e.value.status == abi.ERR_INVALID
        same = st.up(np.frombuffer(ks[0] + ks[0], np.uint8))  # (equal neighbours are not ascending either)
        with pytest.raises(_lib.TsqError, match="index keys not ascending"):
            D.DupChecker(ctx, [hs, D.IndexStream(same.p, offs.p, 2 * len(ks[0]), two.p, 2)], abi.DUP_INSERT)
        bad_offs = st.up(np.array([0, 40, 20], np.int64))
        with pytest.raises(_lib.TsqError, match="offsets decrease or leave the keys"):
            D.DupChecker(ctx, [hs, D.IndexStream(raw.p, bad_offs.p, len(ks[0]) + len(ks[1]), two.p, 2)], abi.DUP_INSERT)
        with pytest.raises(_lib.TsqError, match="table handles not ascending"):
            D.DupChecker(ctx, [D.HandleStream(two.p, 2), ix], abi.DUP_REPLACE)
        # REPLACE over a unique index with a DOUBLE column; INSERT takes it
        fx = D.IndexStream(ix.keys, ix.key_offsets, ix.key_bytes, ix.handles, ix.n, float_key=True)
        with pytest.raises(_lib.TsqError, match="FLOAT / DOUBLE") as e:
            D.DupChecker(ctx, [hs, fx], abi.DUP_REPLACE)
        assert e.value.status == abi.ERR_UNSUPPORTED
        D.DupChecker(ctx, [hs, fx], abi.DUP_INSERT).close()
        # the order of calls, and everything after cancel
        chk = st.checker(abi.DUP_INSERT)
        with pytest.raises(_lib.TsqError, match="INSERT mode"):
            chk.resolve(two.p, 0, two.p, two.p, None, None, None, 0)
        assert chk.match_insert().row == 1
        with pytest.raises(_lib.TsqError, match="called twice"):
            chk.match_insert()
        chk.close()
        chk = st.checker(abi.DUP_REPLACE)
        with pytest.raises(_lib.TsqError, match="before tsq_dupcheck_match"):
            chk.resolve(two.p, 0, two.p, two.p, None, None, None, 0)
        chk.cancel()
        for call in (lambda: chk.push([st.row_handles, (st.kvs[0].keys, st.kvs[0].key_offsets, st.kvs[0].nbytes, st.kvs[0].distinct)], 2),
                     lambda: chk.match_replace(two.p, two.p, two.p), lambda: chk.resolve(two.p, 0, two.p, two.p, None, None, None, 0)):
            with pytest.raises(_lib.TsqError) as e:
                call()
            assert e.value.status == abi.ERR_CANCELLED
        chk.close()
        # removed-row buffers that are too small: nothing written, the count says what is needed
        with pytest.raises(_lib.TsqError, match="too small") as e:
            st.replace(cap_removed=0)
        assert e.value.status == abi.ERR_INVALID and e.value.needed == 1
    finally:
        st.free()
