"""Reference and inputs for the group-id tests (test_groupid_cpu.py, test_groupid_gpu.py, test_agg_manykeys_gpu.py).

The reference maps the concatenated group-key encoding of a row's key cells (oracle.binding.group_key_encode; a non-NULL string is
compactBytesFlag + varint(len) + bytes, util/codec/codec.go:738-744, as the oracle's partial_update states it) to an id in order of
first occurrence.  Above 5 000 rows a numpy restatement of the encoding takes its place (np_ids); test_groupid_gpu.py checks the
restatement against the oracle encoding on the small inputs first."""
import numpy as np

from tinysql_amd import _abi as abi
from tinysql_amd.chunk import Chunk, Column, StrColumn

COMPACT_BYTES_FLAG = 2


def _varint(n):
    ux = (n << 1) ^ (n >> 63)
    out = bytearray()
    while ux >= 0x80:
        out.append((ux & 0x7f) | 0x80)
        ux >>= 7
    out.append(ux)
    return bytes(out)


def encode_cell(orc, col, row):
    """the group-key bytes of one cell"""
    if col.tp == abi.BYTES and not col.IsNull(row):
        v = col.values()[row]
        return bytes([COMPACT_BYTES_FLAG]) + _varint(len(v)) + v
    if col.tp == abi.BYTES:  # NULL: NilFlag, whatever the type
        return orc.group_key_encode(Column(abi.I64, [0], [False]), 0)
    return orc.group_key_encode(col, row)


def oracle_ids(orc, key_cols):
    """ids in first-occurrence order from the oracle's encoding (small inputs)"""
    n = len(key_cols[0])
    str_vals = [c.values() if c.tp == abi.BYTES else None for c in key_cols]
    seen, ids = {}, np.zeros(n, np.uint64)
    nil = orc.group_key_encode(Column(abi.I64, [0], [False]), 0)
    for r in range(n):
        parts = []
        for c, sv in zip(key_cols, str_vals):
            if sv is not None:
                v = sv[r]
                parts.append(nil if v is None else bytes([COMPACT_BYTES_FLAG]) + _varint(len(v)) + v)
            else:
                parts.append(orc.group_key_encode(c, r))
        ids[r] = seen.setdefault(b"".join(parts), len(seen))
    return ids


def _images(col):
    """(flag, image) per row: equal pairs <=> equal group-key encodings of the cells.  flag 0 = NULL (image 0)."""
    n = len(col)
    nn = np.ones(n, bool) if col.notnull is None else col.notnull
    if col.tp == abi.BYTES:
        codes, img = {}, np.zeros(n, np.uint64)
        for r, v in enumerate(col.values()):
            if v is not None:
                img[r] = codes.setdefault(v, len(codes))  # bytes compare by length and content
    elif col.tp in (abi.F32, abi.F64):
        f = col.data.astype(np.float64)  # F32 is widened (exactly)
        u = f.view(np.uint64)
        img = np.where(f >= 0, u | np.uint64(1 << 63), ~u)  # util/codec/float.go:22-30; -0.0 >= 0 is true, NaN >= 0 is false
    else:
        img = col.data.view(np.uint64).copy()  # the 8 bytes; the UNSIGNED flag is ignored
    img = np.where(nn, img, np.uint64(0))
    return nn.astype(np.uint64), img


def np_ids(key_cols):
    """the numpy restatement: ids in first-occurrence order"""
    n = len(key_cols[0])
    m = np.zeros((n, 2 * len(key_cols)), np.uint64)
    for c, col in enumerate(key_cols):
        m[:, 2 * c], m[:, 2 * c + 1] = _images(col)
    _, first, inv = np.unique(m, axis=0, return_index=True, return_inverse=True)
    order = np.argsort(first, kind="stable")
    rank = np.zeros(len(first), np.uint64)
    rank[order] = np.arange(len(first), dtype=np.uint64)
    return rank[inv.reshape(-1)]


def first_rows(ids):
    """row index of the first occurrence of every id, in id order"""
    _, first = np.unique(ids, return_index=True)
    return first


def take(col, idx):
    """the rows `idx` of a column, as a column (the expected dictionary column)"""
    if col.tp == abi.BYTES:
        v = col.values()
        return StrColumn([v[i] for i in idx])
    return Column(col.tp, col.data[idx], None if col.notnull is None else col.notnull[idx])


# ---------------------------------------------------------------- inputs
COLSETS = ["i64", "mixed", "bytes_first", "bytes_mid", "bytes_last", "nulls5", "allnull"]
KEYSETS = ["one", "sqrt", "distinct", "lastcol", "perm"]


def _key_matrix(rng, rows, n_keys, keyset):
    k = np.zeros((rows, n_keys), np.int64)
    g = int(np.ceil(np.sqrt(rows)))
    if keyset == "sqrt":
        grp = rng.integers(0, g, rows)
        for c in range(n_keys):
            k[:, c] = (grp * (c + 3) + c) % 1000003
    elif keyset == "distinct":
        grp = rng.permutation(rows)
        for c in range(n_keys):
            k[:, c] = grp if c == 0 else (grp * (c + 1) + c) % 65521
    elif keyset == "lastcol":  # keys that differ only in the last column
        k[:, :] = 7
        k[:, n_keys - 1] = rng.integers(0, g + 1, rows)
    elif keyset == "perm":  # keys that are column permutations (rotations) of each other
        grp, rot = rng.integers(0, max(1, g // 4 + 1), rows), rng.integers(0, n_keys, rows)
        for c in range(n_keys):
            k[:, c] = 10 + (c + rot) % n_keys + 100 * grp
    return k


def _typed(rng, tp, v, null_frac):
    n = len(v)
    nn = None if null_frac == 0 else rng.random(n) >= null_frac
    if tp == abi.BYTES:
        vals = [(b"k%d" % x) * (int(x) % 3 + 1) for x in v.tolist()]
        if nn is not None:
            vals = [s if keep else None for s, keep in zip(vals, nn)]
        return StrColumn(vals)
    if tp in (abi.F32, abi.F64):
        f = v.astype(np.float64)
        zero = (v % 7) == 3  # some cells become +0.0 / -0.0 by row parity: one group
        f[zero] = np.where(np.arange(n)[zero] % 2 == 0, 0.0, -0.0)
        return Column(tp, f, nn)
    if tp == abi.U64:
        return Column(tp, v.astype(np.uint64) + np.uint64(1 << 63), nn)
    return Column(tp, v - 40, nn)


def make_keys(rows, n_keys, colset, keyset, seed=0):
    """key columns (a list of Column / StrColumn) of one test input"""
    rng = np.random.default_rng(1000 * seed + 7 * rows + n_keys)
    k = _key_matrix(rng, rows, n_keys, keyset)
    types = [abi.I64] * n_keys
    null_frac = 0.0
    if colset in ("mixed", "nulls5"):
        cyc = [abi.I64, abi.U64, abi.F32, abi.F64]
        types = [cyc[c % 4] for c in range(n_keys)]
        if colset == "nulls5":
            null_frac = 0.05
            if n_keys >= 5:
                types[n_keys - 1] = abi.BYTES
    elif colset.startswith("bytes_"):
        types[{"first": 0, "mid": n_keys // 2, "last": n_keys - 1}[colset[6:]]] = abi.BYTES
    cols = [_typed(rng, types[c], k[:, c], null_frac) for c in range(n_keys)]
    if colset == "allnull":
        c = n_keys // 2
        cols[c] = Column(abi.I64, np.zeros(rows, np.int64), np.zeros(rows, bool))
    return cols
