"""The yardstick of join keys and GROUP BY keys at their edge values: named edge cells per key type, and a plain statement of which
two cells are equal as join keys and which cells share a group.  No GPU and no oracle in here: Python ints and bit patterns through
struct / numpy.  (tests/agg_edge.py does the same for the aggregates' ARGUMENT cells; there the keys are ordinary small integers.)

Join keys — codec.EqualChunkRow, util/codec/codec.go:363-382: two non-NULL cells are equal iff they carry the same flag and the same
bytes; a NULL cell equals nothing (executor/hash_table.go:161-163 never inserts it, join.go:344 never probes with it).  The flag and
the 8 bytes of a cell are encodeHashChunkRowIdx's, codec.go:212-240:
  integers       flag 8 (varintFlag), the raw 8 bytes                                              codec.go:218-219, 225
  UNSIGNED       flag 9 (uvarintFlag) when the cell read as int64 is negative, i.e. >= 2^63        codec.go:220-224
  float32        flag 5 (floatFlag), the bytes of the cell WIDENED to float64                      codec.go:226-229
  float64        flag 5, the raw 8 bytes                                                           codec.go:230-232
The bytes are compared, not the numbers: -0.0 != +0.0, a NaN equals the NaN with the same bits and no other.

GROUP BY keys — codec.HashGroupKey, codec.go:713-746: the group of a row is the byte string of its key cells.
  integers       encodeSignedInt of the cell's int64 (codec.go:715-723): the UNSIGNED flag plays no part, the 64 bits decide
  reals          floatFlag + EncodeFloat (codec.go:724-733), whose image is encodeFloatToCmpUint64, util/codec/float.go:22-30:
                 `if f >= 0 { u |= signMask } else { u = ^u }`.  -0.0 >= 0 holds: both zeros have the image 0x8000000000000000.
                 NaN >= 0 does not hold: EVERY NaN takes the ^u branch.  One with the sign bit clear, 0x7ff8000000000000 + p, gets the
                 image 0x8007ffffffffffff - p: the top bit is set, and it is also the image of the positive denormal
                 0x0007ffffffffffff - p.  The reference puts the two in one group (and 0x7fffffffffffffff with the zeros) and outputs
                 the first row's own cell for FIRST_ROW(key) (executor/aggfuncs/func_first_row.go:67-81).  decodeCmpUintToFloat
                 (float.go:32-40) would turn such an image into the denormal: the image is not invertible there.
  NULL           NilFlag (codec.go:718-719, 727-728): the NULL keys are one group
  (a float32 key column: this project widens the cell and groups by the image of the double, tsq_agg.hip group_key_word)

A cell is None (NULL), an int (I64: -2^63 .. 2^63-1, U64: 0 .. 2^64-1) or a float (F64; an F32 cell holds the widened value, which is
exactly representable in 32 bits).  No signalling float32 NaN is on the grid: the widening conversion quiets it in hardware
(cvtss2sd, v_cvt_f64_f32), so its bits as a double depend on where the conversion ran, and no rule of the reference is at stake.
"""
import struct

import numpy as np

from tinysql_amd import _abi as abi
from tinysql_amd.chunk import Column

from . import helpers as H

M64 = (1 << 64) - 1
I64_MIN, I64_MAX, U64_MAX = -(1 << 63), (1 << 63) - 1, (1 << 64) - 1
SIGN = 1 << 63
SENT = 0x8080808080808080            # the join table's EMPTY sentinel (tsq_jointable.h): a legal key
TYPES = {"i64": abi.I64, "u64": abi.U64, "f64": abi.F64, "f32": abi.F32}
INT_TYPES, REAL_TYPES = ("i64", "u64"), ("f64", "f32")
FLAG_INT, FLAG_UINT, FLAG_FLOAT = 8, 9, 5  # codec.go:36-49


def f64_from_bits(b):
    return struct.unpack("<d", struct.pack("<Q", b))[0]


def f64_bits(v):
    return struct.unpack("<Q", struct.pack("<d", v))[0]


def f32_from_bits(b):
    """the float32 with these bits, widened (exact; a quiet NaN keeps its sign and its payload, shifted by 29 bits)"""
    return float(np.array([b], dtype=np.uint32).view(np.float32)[0])


def _signed(w):
    return w - (1 << 64) if w >> 63 else w


# ---------------------------------------------------------------------------------------------------------------- the edge cells
EDGE = {
    "i64": [
        ("min", I64_MIN), ("min+1", I64_MIN + 1), ("-2^31", -(1 << 31)), ("-1", -1), ("0", 0), ("1", 1), ("2^31-1", (1 << 31) - 1),
        ("2^31", 1 << 31), ("2^32", 1 << 32), ("max-1", I64_MAX - 1), ("max", I64_MAX),
        ("sentinel", _signed(SENT)), ("unmix(sentinel)", H.unmix64(SENT)),
    ],
    "u64": [
        ("0", 0), ("1", 1), ("2^63-1", (1 << 63) - 1), ("2^63", 1 << 63), ("2^63+1", (1 << 63) + 1), ("max-1", U64_MAX - 1), ("max", U64_MAX),
        ("sentinel", SENT),
    ],
    "f64": [(n, f64_from_bits(b)) for n, b in [
        ("+0", 0x0000000000000000), ("-0", 0x8000000000000000),
        ("+denorm_min", 0x0000000000000001), ("-denorm_min", 0x8000000000000001),
        ("denorm_7ffff", 0x0007FFFFFFFFFFFF),                     # shares its image with the NaN 0x7ff8000000000000
        ("+dbl_min", 0x0010000000000000), ("-dbl_min", 0x8010000000000000),
        ("0.1", f64_bits(0.1)), ("0.1f", f64_bits(f32_from_bits(0x3DCCCCCD))),
        ("1", f64_bits(1.0)), ("-1", f64_bits(-1.0)), ("1.5", f64_bits(1.5)),
        ("2^24", f64_bits(16777216.0)), ("2^24+1", f64_bits(16777217.0)),
        ("+dbl_max", 0x7FEFFFFFFFFFFFFF), ("-dbl_max", 0xFFEFFFFFFFFFFFFF),
        ("+inf", 0x7FF0000000000000), ("-inf", 0xFFF0000000000000),
        ("nan", 0x7FF8000000000000), ("nan_p1", 0x7FF8000000000001), ("-nan", 0xFFF8000000000000),
        ("nan_pos_ones", 0x7FFFFFFFFFFFFFFF), ("nan_neg_ones", 0xFFFFFFFFFFFFFFFF), ("snan", 0x7FF0000000000001),
    ]],
    "f32": [(n, f32_from_bits(b)) for n, b in [
        ("+0", 0x00000000), ("-0", 0x80000000), ("+denorm_min", 0x00000001), ("-denorm_min", 0x80000001),
        ("0.1f", 0x3DCCCCCD), ("2^24-1", 0x4B7FFFFF), ("2^24", 0x4B800000), ("2^24+2", 0x4B800001),
        ("+flt_max", 0x7F7FFFFF), ("-flt_max", 0xFF7FFFFF), ("+inf", 0x7F800000), ("-inf", 0xFF800000),
        ("nan", 0x7FC00000), ("nan_p1", 0x7FC00001), ("-nan", 0xFFC00000),
    ]],
}
TYPE_NAMES = tuple(EDGE)


def cells(tp):
    return [c for _, c in EDGE[tp]]


def key_bits(tp, cell):
    """the 64 bits a non-NULL cell contributes to either rule: the integer's two's complement, the (widened) double's bits"""
    if tp in INT_TYPES:
        assert (I64_MIN <= cell <= I64_MAX) if tp == "i64" else (0 <= cell <= U64_MAX), (tp, cell)
        return cell & M64
    return f64_bits(cell)


def own_bits(tp, cell):
    """the bit pattern of a cell in the width of its column (F32: 32 bits)"""
    if tp == "f32":
        return int(column(tp, [cell]).data.view(np.uint32)[0])
    return key_bits(tp, cell)


def column(tp, cs):
    """a Column of type tp holding the cells, bit for bit (asserted: a NaN keeps its sign and payload on the way through numpy)"""
    nn = np.array([c is not None for c in cs], dtype=bool)
    if tp in INT_TYPES:
        data = np.array([0 if c is None else c & M64 for c in cs], dtype=np.uint64)
        data = data.view(np.int64) if tp == "i64" else data
    else:
        data = np.array([0 if c is None else f64_bits(c) for c in cs], dtype=np.uint64).view(np.float64)
        if tp == "f32":
            wide = data
            data = wide.astype(np.float32)
            assert (data.astype(np.float64).view(np.uint64) == wide.view(np.uint64)).all(), "a cell that is no widened float32"
    return Column(TYPES[tp], data, nn if not nn.all() else None)


def cells_of_column(tp, col):
    """the inverse of column(): the cells of a Column (None for NULL)"""
    nn = col.notnull if col.notnull is not None else np.ones(len(col), bool)
    if tp in INT_TYPES:
        vals = [int(v) for v in col.data]
    else:
        vals = [f64_from_bits(int(b)) for b in np.asarray(col.data).astype(np.float64).view(np.uint64)]
    return [v if ok else None for v, ok in zip(vals, nn)]


# ---------------------------------------------------------------------------------------------------------------- join keys
def join_flag_word(tp, cell):
    """(flag, the 8 bytes as a 64-bit word) of a non-NULL key cell: codec.go:212-240"""
    w = key_bits(tp, cell)
    if tp in REAL_TYPES:
        return (FLAG_FLOAT, w)
    return (FLAG_UINT if tp == "u64" and w >> 63 else FLAG_INT, w)


def join_equal(tpa, a, tpb, b):
    """codec.go:363-382: same flag, same bytes; NULL equals nothing"""
    return a is not None and b is not None and join_flag_word(tpa, a) == join_flag_word(tpb, b)


def join_pairs(tpb, build, tpp, probe, equal=join_equal):
    """the (probe row, build row) pairs of an inner join of the two key columns, in probe order, build rows ascending.
    `equal`: the key rule (the tests that show the comparison bites pass a wrong one)."""
    if equal is join_equal:  # (the same pairs through an index: the tables of the GPU tests have thousands of rows)
        index = {}
        for j, b in enumerate(build):
            if b is not None:
                index.setdefault(join_flag_word(tpb, b), []).append(j)
        return [(i, j) for i, p in enumerate(probe) if p is not None for j in index.get(join_flag_word(tpp, p), ())]
    return [(i, j) for i, p in enumerate(probe) for j, b in enumerate(build) if equal(tpp, p, tpb, b)]


def pairs_mismatch(want, got):
    """"" when the two lists hold the same pairs as multisets, else what differs"""
    w, g = sorted(want), sorted(got)
    if w == g:
        return ""
    ws, gs = set(w), set(g)
    return "pairs missing: %s, pairs too many: %s, %d / %d pairs" % (sorted(ws - gs)[:4], sorted(gs - ws)[:4], len(g), len(w))


# ---------------------------------------------------------------------------------------------------------------- group keys
def group_image(tp, cell):
    """the 64-bit image two non-NULL cells of a GROUP BY column share iff they are one group (None for NULL)"""
    if cell is None:
        return None
    if tp in INT_TYPES:
        return key_bits(tp, cell)          # codec.go:715-723
    u = f64_bits(cell)
    return (u | SIGN) if cell >= 0 else (~u & M64)  # float.go:22-30 (`cell >= 0` is false for every NaN, true for -0.0)


def groups_of(tp, cs, image=group_image):
    """{image (None: the NULL keys): [row numbers]} — the partition of the rows into groups, rows ascending"""
    out = {}
    for i, c in enumerate(cs):
        out.setdefault(image(tp, c), []).append(i)
    return out


def groups_mismatch(want, got_rowsets):
    """`want`: groups_of(..); `got_rowsets`: an iterable of row-number collections, one per output group.  "" or what differs."""
    w = sorted(tuple(sorted(r)) for r in want.values())
    g = sorted(tuple(sorted(r)) for r in got_rowsets)
    if w == g:
        return ""
    return "groups missing: %s, groups too many: %s" % ([x for x in w if x not in g][:4], [x for x in g if x not in w][:4])


def agg_mismatch(tp, cs, args, out_rows, image=group_image):
    """out_rows: the rows (FIRST_ROW(key), COUNT(*), SUM(arg), MIN(arg)) of an aggregate over the key cells `cs` and the integer
    arguments `args` (no NULL among them).  "" when they are exactly the groups of groups_of — every group once, with its exact count,
    sum and minimum, and a key whose bits are those of one of the group's own cells (either zero for the zeros, that NaN's own bits
    for a NaN, either cell where a NaN and a denormal share an image) — else what differs."""
    want = groups_of(tp, cs, image)
    seen = set()
    for row in out_rows:
        key, cnt, s, mn = row
        img = image(tp, key)
        if img not in want:
            return "a group with the key %r (image %r) that no row has" % (key, img)
        if img in seen:
            return "the group of image %r comes out twice" % (img,)
        seen.add(img)
        rows = want[img]
        exp = (len(rows), sum(args[i] for i in rows), min(args[i] for i in rows))
        if (int(cnt), int(s), int(mn)) != exp:
            return "group of %r: (count, sum, min) = %r, want %r" % (key, (int(cnt), int(s), int(mn)), exp)
        if key is not None and own_bits(tp, key) not in {own_bits(tp, cs[i]) for i in rows}:
            return "group of image %x: the key %r (bits %x) is no cell of the group: %s" % (
                img, key, own_bits(tp, key), sorted("%x" % own_bits(tp, cs[i]) for i in rows)[:6])
    if len(seen) != len(want):
        return "%d groups are missing, e.g. image %r" % (len(want) - len(seen), sorted(set(want) - seen, key=str)[0])
    return ""
