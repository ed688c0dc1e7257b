"""ctypes mirror of include/tsq.h (struct layouts, enums).  Pure declarations — no library loading.

Shared by the product binding (tinysql_amd._lib) and by the test-only oracle binding
(tests/oracle_binding.py), so both sides are driven by byte-identical structs.
"""
import ctypes as C

TSQ_ABI_VERSION = 10
RADIX_AUTO, RADIX_OFF, RADIX_FORCE = -1, 0, 1
AGGFAST_AUTO, AGGFAST_OFF, AGGFAST_FORCE = -1, 0, 1
JIT_AUTO, JIT_OFF, JIT_FORCE = -1, 0, 1

# status codes
OK, ERR_INVALID, ERR_UNSUPPORTED, ERR_OOM_DEVICE, ERR_HIP = 0, 1, 2, 3, 4
ERR_OVERFLOW_BIGINT, ERR_OVERFLOW_BIGINT_UNSIGNED, ERR_OVERFLOW_DOUBLE = 5, 6, 7
ERR_CANCELLED, ERR_NO_DEVICE, ERR_DIV_BY_ZERO = 8, 9, 10
ERR_TRUNCATED_WRONG_VALUE = 11  # ABI 8
ERR_DATA_TOO_LONG, ERR_OUT_OF_RANGE, ERR_BAD_NULL, ERR_BAD_UTF8 = 12, 13, 14, 15  # tsq_cast_run / tsq_autoid_fill
ERR_KEY_EXISTS = 16  # tsq_dupcheck_match: kv.ErrKeyExists
ERR_LOCKED = 17  # tsq_mvcc_scan: mocktikv.ErrLocked
# tsq_expr_prog.str_ctx (ABI 8): the statement's string-to-int flags, 0 = a SELECT
STRCTX_NOT_STRICT, STRCTX_TRUNCATE_ERROR, STRCTX_IGNORE_TRUNCATE, STRCTX_EMPTY_NOT_ZERO = 1, 2, 4, 8
STATUS_NAMES = {
    0: "OK", 1: "INVALID", 2: "UNSUPPORTED", 3: "OOM_DEVICE", 4: "HIP", 5: "OVERFLOW_BIGINT",
    6: "OVERFLOW_BIGINT_UNSIGNED", 7: "OVERFLOW_DOUBLE", 8: "CANCELLED", 9: "NO_DEVICE", 10: "DIV_BY_ZERO", 11: "TRUNCATED_WRONG_VALUE",
    12: "DATA_TOO_LONG", 13: "OUT_OF_RANGE", 14: "BAD_NULL", 15: "BAD_UTF8", 16: "KEY_EXISTS",
    17: "LOCKED",
}

# column types
I64, U64, F32, F64, BYTES = 0, 1, 2, 3, 4
COL_DEVICE = 1
COL_BORROW = 2
COL_RETAIN = 4

# generator kinds
GEN_SEQ, GEN_AFFINE, GEN_RAND_MOD, GEN_RAND_F64, GEN_HASH_OF_COL, GEN_ZIPF_OCT = 0, 1, 2, 3, 4, 5

# join types / agg funcs / modes
JOIN_INNER, JOIN_LEFT_OUTER, JOIN_RIGHT_OUTER = 0, 1, 2
AGG_COUNT, AGG_SUM, AGG_AVG, AGG_MAX, AGG_MIN, AGG_FIRSTROW = 0, 1, 2, 3, 4, 5
MODE_COMPLETE, MODE_FINAL, MODE_PARTIAL1, MODE_PARTIAL2 = 0, 1, 2, 3

MAX_KEYS, MAX_COLS, MAX_AGGS, MAX_GROUP_KEYS = 4, 16, 16, 4
GROUPID_MAX_KEYS = 16  # tsq_groupid_* / tsq_agg_create_keys
EXPR_MAX_OPS, EXPR_MAX_STACK, EXPR_MAX_CONSTS, EXPR_STR_POOL = 64, 12, 32, 256

# opcodes
OP_COL_INT, OP_COL_REAL, OP_CONST_INT, OP_CONST_REAL, OP_CONST_NULL_INT, OP_CONST_NULL_REAL = 1, 2, 3, 4, 5, 6
OP_PLUS_REAL, OP_MINUS_REAL, OP_MUL_REAL, OP_DIV_REAL = 10, 11, 12, 13
OP_PLUS_INT, OP_MINUS_INT, OP_MUL_INT, OP_MUL_INT_UNSIGNED = 14, 15, 16, 17
OP_LT_INT, OP_LE_INT, OP_GT_INT, OP_GE_INT, OP_EQ_INT, OP_NE_INT = 20, 21, 22, 23, 24, 25
OP_LT_REAL, OP_LE_REAL, OP_GT_REAL, OP_GE_REAL, OP_EQ_REAL, OP_NE_REAL = 26, 27, 28, 29, 30, 31
OP_LOGIC_AND, OP_LOGIC_OR, OP_NOT_INT, OP_NOT_REAL, OP_NEG_INT, OP_NEG_REAL = 40, 41, 42, 43, 44, 45
OP_ISNULL_INT, OP_ISNULL_REAL = 46, 47
OP_IFNULL_INT, OP_IFNULL_REAL, OP_IF_INT, OP_IF_REAL = 50, 51, 52, 53
OP_IN_INT, OP_IN_REAL = 60, 61
OP_COL_STR, OP_CONST_STR, OP_CONST_NULL_STR = 70, 71, 72
OP_LT_STR, OP_LE_STR, OP_GT_STR, OP_GE_STR, OP_EQ_STR, OP_NE_STR = 73, 74, 75, 76, 77, 78
OP_STRCMP, OP_LENGTH, OP_ISNULL_STR, OP_IFNULL_STR, OP_IF_STR, OP_IN_STR = 79, 80, 81, 82, 83, 84
F_LHS_UNSIGNED, F_RHS_UNSIGNED, F_FORCE_SIGNED = 1, 2, 4


RC_HANDLE, RC_HAS_DEFAULT, RC_BIT = 1, 2, 4  # tsq_rowcodec_col.flags (a bit column: its byte size in bits 8..11)
ENC_COMPARABLE = 1  # tsq_rows_encode col_flags
IDX_UNIQUE = 1  # tsq_indexkeys_encode index_flags
AN_RAW = 2  # tsq_analyze_cfg.col_flags: the cells of a TSQ_BYTES column already are the datum bytes
AN_WRAP_BYTES = 1  # tsq_analyze_cfg.flags: the FM sketch hashes the bytes datum of the encoded value
AN_MAX_CM_COUNTERS = 16384


class RowcodecCol(C.Structure):
    """tsq_rowcodec_col — one requested column of a stored-row scan (rowcodec.ColInfo, util/rowcodec/decoder.go:45-55)."""
    _fields_ = [
        ("col_id", C.c_int64),
        ("type", C.c_int32),
        ("flags", C.c_uint32),
        ("def_bits", C.c_uint64),
        ("def_bytes", C.c_void_p),
        ("def_len", C.c_int64),
    ]


# tsq_cast_col.tp (mysql.Type*), .flags, the statement flags of tsq_cast_create, the flag of tsq_autoid_fill
(TP_TINY, TP_SHORT, TP_LONG, TP_FLOAT, TP_DOUBLE, TP_LONGLONG, TP_INT24, TP_VARCHAR, TP_BIT, TP_TINY_BLOB, TP_MEDIUM_BLOB, TP_LONG_BLOB, TP_BLOB,
 TP_VAR_STRING, TP_STRING) = 1, 2, 3, 4, 5, 8, 9, 15, 16, 249, 250, 251, 252, 253, 254
CAST_UNSIGNED, CAST_NOT_NULL, CAST_AUTO_INCREMENT, CAST_CHARSET_BIN, CAST_CHARSET_UTF8, CAST_CHARSET_UTF8MB4, CAST_DEFAULT_NULL = 1, 2, 4, 8, 16, 32, 64
CAST_IGNORE_TRUNCATE, CAST_TRUNCATE_AS_WARNING, CAST_OVERFLOW_AS_WARNING, CAST_BAD_NULL_AS_WARNING, CAST_IN_INSERT, CAST_SKIP_UTF8_CHECK = 1, 2, 4, 8, 16, 32
AUTOID_NO_AUTO_VALUE_ON_ZERO = 1


# tsq_dupcheck_*: stream kinds, modes, the stream flag
DUP_MAX_STREAMS = 8
DUP_HANDLE, DUP_INDEX = 0, 1
DUP_INSERT, DUP_REPLACE = 0, 1
DUP_FLOAT_KEY = 1


class DupStream(C.Structure):
    """tsq_dup_stream — one key that must be unique, with the store's entries of it."""
    _fields_ = [("kind", C.c_int32), ("flags", C.c_uint32), ("handles", C.c_void_p), ("n", C.c_int64), ("keys", C.c_void_p), ("key_offsets", C.c_void_p),
                ("key_bytes", C.c_int64)]


class DupKeys(C.Structure):
    """tsq_dup_keys — one stream's part of a push: the rows' handles, or their encoded index keys with the distinct flags."""
    _fields_ = [("handles", C.c_void_p), ("keys", C.c_void_p), ("key_offsets", C.c_void_p), ("key_bytes", C.c_int64), ("distinct", C.c_void_p)]


class DupConflict(C.Structure):
    """tsq_dup_conflict — INSERT mode's first error."""
    _fields_ = [("row", C.c_int64), ("stream", C.c_int32), ("from_store", C.c_int32), ("dup_handle", C.c_int64), ("dup_row", C.c_int64)]


class DupResult(C.Structure):
    """tsq_dup_result — the host-side counts of tsq_dupcheck_resolve."""
    _fields_ = [("affected", C.c_int64), ("n_added", C.c_int64), ("n_put", C.c_int64), ("n_removed_store", C.c_int64), ("n_removed_batch", C.c_int64),
                ("rowid_base", C.c_int64)]


# tsq_mvcc_*: value types (mvcc.go:30-34), lock ops (kvrpcpb.Op), the range flag
MVCC_PUT, MVCC_DELETE, MVCC_ROLLBACK = 0, 1, 2
MVCC_OP_PUT, MVCC_OP_DEL, MVCC_OP_LOCK, MVCC_OP_ROLLBACK = 0, 1, 2, 3
MVCC_POINT = 1


class MvccData(C.Structure):
    """tsq_mvcc_data — the versions and the locks of a store, decoded, in the reference's LevelDB order."""
    _fields_ = [("keys", C.c_void_p), ("key_offsets", C.c_void_p), ("key_bytes", C.c_int64), ("commit_ts", C.c_void_p), ("start_ts", C.c_void_p),
                ("types", C.c_void_p), ("values", C.c_void_p), ("value_offsets", C.c_void_p), ("value_bytes", C.c_int64), ("n", C.c_int64),
                ("lock_keys", C.c_void_p), ("lock_key_offsets", C.c_void_p), ("lock_key_bytes", C.c_int64), ("lock_start_ts", C.c_void_p),
                ("lock_ttl", C.c_void_p), ("lock_ops", C.c_void_p), ("lock_primaries", C.c_void_p), ("lock_primary_offsets", C.c_void_p),
                ("lock_primary_bytes", C.c_int64), ("n_locks", C.c_int64), ("data_flags", C.c_uint32), ("reserved", C.c_uint32)]


class MvccResult(C.Structure):
    """tsq_mvcc_result — the host-side counts of tsq_mvcc_scan."""
    _fields_ = [("n_pairs", C.c_int64), ("key_bytes", C.c_int64), ("value_bytes", C.c_int64), ("positions", C.c_int64)]


# tsq_mvcc_prewrite / commit / rollback: the verdict of one key
MVCC_V_OK, MVCC_V_NOOP, MVCC_V_LOCKED, MVCC_V_CONFLICT, MVCC_V_TXN_NOT_FOUND, MVCC_V_ALREADY_COMMITTED = 0, 1, 2, 3, 4, 5


class MvccWriteReq(C.Structure):
    """tsq_mvcc_write_req — the keys of one Prewrite / Commit / Rollback (strictly ascending), a prewrite's ops and values."""
    _fields_ = [("keys", C.c_void_p), ("key_offsets", C.c_void_p), ("key_bytes", C.c_int64), ("n_keys", C.c_int64), ("ops", C.c_void_p),
                ("values", C.c_void_p), ("value_offsets", C.c_void_p), ("value_bytes", C.c_int64), ("primary", C.c_void_p), ("primary_len", C.c_int64),
                ("start_ts", C.c_uint64), ("commit_ts", C.c_uint64), ("ttl", C.c_uint64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


class MvccWriteResult(C.Structure):
    """tsq_mvcc_write_result — the counts of one write call."""
    _fields_ = [("n_errors", C.c_int64), ("first_error", C.c_int64), ("versions_added", C.c_int64), ("versions_replaced", C.c_int64),
                ("locks_added", C.c_int64), ("locks_removed", C.c_int64), ("kernel_ms", C.c_double)]


class MvccStoreSizes(C.Structure):
    """tsq_mvcc_store_sizes — what tsq_mvcc_export needs room for."""
    _fields_ = [("n", C.c_int64), ("n_locks", C.c_int64), ("key_bytes", C.c_int64), ("value_bytes", C.c_int64), ("lock_key_bytes", C.c_int64),
                ("lock_primary_bytes", C.c_int64), ("lock_value_bytes", C.c_int64)]


MVCC_ARRAY_NAMES = ("keys", "key_offsets", "commit_ts", "start_ts", "types", "values", "value_offsets", "lock_keys", "lock_key_offsets", "lock_start_ts",
                    "lock_ttl", "lock_ops", "lock_primaries", "lock_primary_offsets", "lock_values", "lock_value_offsets")


class MvccArrays(C.Structure):
    """tsq_mvcc_arrays — the caller's device buffers of tsq_mvcc_export."""
    _fields_ = [(name, C.c_void_p) for name in MVCC_ARRAY_NAMES]


class MvccLockScan(C.Structure):
    """tsq_mvcc_lock_scan — the counts of tsq_mvcc_scan_lock, which size its fetch."""
    _fields_ = [("n_locks", C.c_int64), ("key_bytes", C.c_int64), ("primary_bytes", C.c_int64), ("kernel_ms", C.c_double)]


class MvccMaintResult(C.Structure):
    """tsq_mvcc_maint_result — the counts of tsq_mvcc_resolve_lock / gc / delete_range."""
    _fields_ = [("versions_added", C.c_int64), ("versions_replaced", C.c_int64), ("versions_removed", C.c_int64), ("locks_removed", C.c_int64),
                ("n_errors", C.c_int64), ("first_error", C.c_int64), ("kernel_ms", C.c_double), ("mark_ms", C.c_double)]


class MembufCfg(C.Structure):
    """tsq_membuf_cfg — the limits of a transaction buffer (kv.TxnEntrySizeLimit / TxnTotalSizeLimit; 0 = none)."""
    _fields_ = [("entry_size_limit", C.c_int64), ("total_size_limit", C.c_int64), ("flags", C.c_uint32), ("reserved", C.c_uint32)]


# tsq_membuf_push: the kind of a push's entries; the values are TSQ_MVCC_OP_PUT / DEL / LOCK's
MEMBUF_SET, MEMBUF_DELETE, MEMBUF_LOCK = 0, 1, 2


class MembufResult(C.Structure):
    """tsq_membuf_result — the counts of tsq_membuf_finish."""
    _fields_ = [("n_entries", C.c_int64), ("puts", C.c_int64), ("dels", C.c_int64), ("locks", C.c_int64), ("size", C.c_int64),
                ("primary_index", C.c_int64), ("sort_passes", C.c_int64), ("kernel_ms", C.c_double)]


class MembufScanResult(C.Structure):
    """tsq_membuf_scan_result — the counts of tsq_membuf_scan / tsq_membuf_scan_points, which size tsq_membuf_fetch."""
    _fields_ = [("n_pairs", C.c_int64), ("key_bytes", C.c_int64), ("value_bytes", C.c_int64), ("positions", C.c_int64), ("skipped_dels", C.c_int64)]


class UnionStoreResult(C.Structure):
    """tsq_unionstore_result — the counts of tsq_unionstore_scan / tsq_unionstore_get, which size tsq_unionstore_fetch."""
    _fields_ = [("n_pairs", C.c_int64), ("key_bytes", C.c_int64), ("value_bytes", C.c_int64), ("positions_snapshot", C.c_int64), ("positions_buffer", C.c_int64),
                ("shadowed", C.c_int64), ("skipped_dels", C.c_int64), ("dangling_dels", C.c_int64), ("from_buffer", C.c_int64)]


UNION_ROUTE_NONE, UNION_ROUTE_MERGE, UNION_ROUTE_SNAPSHOT, UNION_ROUTE_POINTS = 0, 1, 2, 3


class CastCol(C.Structure):
    """tsq_cast_col — one column of the table an INSERT .. SELECT writes (model.ColumnInfo's FieldType + where its value comes from)."""
    _fields_ = [
        ("src_col", C.c_int32), ("src_type", C.c_int32), ("tp", C.c_int32), ("flen", C.c_int32), ("decimal", C.c_int32), ("flags", C.c_uint32),
        ("def_bits", C.c_uint64), ("def_bytes", C.c_void_p), ("def_len", C.c_int64),
    ]


class Col(C.Structure):
    """tsq_col — mirrors util/chunk/column.go:28-34."""
    _fields_ = [
        ("data", C.c_void_p),
        ("null_bitmap", C.c_void_p),
        ("offsets", C.c_void_p),
        ("length", C.c_int64),
        ("elem_size", C.c_int32),
        ("type", C.c_int32),
        ("flags", C.c_uint32),
        ("reserved", C.c_uint32),
    ]


class GenSpec(C.Structure):
    _fields_ = [
        ("kind", C.c_int32), ("table", C.c_int32), ("col", C.c_int32), ("null_pct", C.c_int32),
        ("seed", C.c_uint64), ("start", C.c_int64), ("a", C.c_uint64), ("b", C.c_uint64), ("m", C.c_uint64),
    ]


class ExprOp(C.Structure):
    _fields_ = [("opcode", C.c_uint8), ("flags", C.c_uint8), ("arg", C.c_uint16), ("aux", C.c_uint32)]


class ExprProg(C.Structure):
    _fields_ = [
        ("n_ops", C.c_int32), ("n_consts", C.c_int32), ("result_type", C.c_int32), ("result_unsigned", C.c_int32),
        ("ops", ExprOp * EXPR_MAX_OPS), ("consts", C.c_int64 * EXPR_MAX_CONSTS),
        ("n_str_bytes", C.c_int32), ("str_ctx", C.c_int32), ("str_pool", C.c_uint8 * EXPR_STR_POOL),
    ]


class JoinCfg(C.Structure):
    _fields_ = [
        ("join_type", C.c_int32), ("build_is_right", C.c_int32), ("n_keys", C.c_int32),
        ("build_key_idx", C.c_int32 * MAX_KEYS), ("probe_key_idx", C.c_int32 * MAX_KEYS),
        ("n_build_cols", C.c_int32), ("n_probe_cols", C.c_int32),
        ("build_types", C.c_int32 * MAX_COLS), ("probe_types", C.c_int32 * MAX_COLS),
        ("est_build_rows", C.c_int64), ("max_chunk_size", C.c_int32), ("concurrency", C.c_int32),
        ("probe_batch_rows", C.c_int64),
        ("other_conds", C.POINTER(ExprProg)), ("n_other_conds", C.c_int32),
        ("outer_filters", C.POINTER(ExprProg)), ("n_outer_filters", C.c_int32),
    ]


class AggFunc(C.Structure):
    _fields_ = [("func", C.c_int32), ("mode", C.c_int32), ("arg_col", C.c_int32), ("arg_col2", C.c_int32),
                ("arg_type", C.c_int32), ("reserved", C.c_int32)]


class AggCfg(C.Structure):
    _fields_ = [
        ("n_group_keys", C.c_int32), ("group_key_col", C.c_int32 * MAX_GROUP_KEYS),
        ("group_key_type", C.c_int32 * MAX_GROUP_KEYS), ("n_aggs", C.c_int32), ("aggs", AggFunc * MAX_AGGS),
        ("n_input_cols", C.c_int32), ("input_types", C.c_int32 * MAX_COLS), ("est_groups", C.c_int64),
        ("max_chunk_size", C.c_int32), ("reserved", C.c_int32),
    ]


class SortCfg(C.Structure):
    _fields_ = [
        ("n_cols", C.c_int32), ("col_types", C.c_int32 * MAX_COLS), ("n_keys", C.c_int32), ("key_col", C.c_int32 * MAX_KEYS),
        ("key_desc", C.c_int32 * MAX_KEYS), ("limit_offset", C.c_int64), ("limit_count", C.c_int64), ("max_chunk_size", C.c_int32),
        ("reserved", C.c_int32),
    ]


class UnionScanCfg(C.Structure):
    """tsq_unionscan_cfg — UnionScanExec: belowHandleIndex, usedIndex, desc (executor/union_scan.go:89-110)."""
    _fields_ = [
        ("n_cols", C.c_int32), ("col_types", C.c_int32 * MAX_COLS), ("handle_col", C.c_int32), ("n_keys", C.c_int32),
        ("key_col", C.c_int32 * MAX_KEYS), ("desc", C.c_int32), ("max_chunk_size", C.c_int32),
    ]


class AnalyzeCfg(C.Structure):
    """tsq_analyze_cfg — the column collector of an ANALYZE request (tipb.AnalyzeColumnsReq: SampleSize, SketchSize, CmsketchDepth / Width)."""
    _fields_ = [
        ("n_cols", C.c_int32), ("col_types", C.c_int32 * MAX_COLS), ("col_flags", C.c_uint32 * MAX_COLS), ("reserved", C.c_int32),
        ("max_sample_size", C.c_int64), ("max_fm_size", C.c_int64), ("cm_depth", C.c_int32), ("cm_width", C.c_int32),
        ("flags", C.c_uint32), ("reserved2", C.c_uint32), ("sample_seed", C.c_uint64),
    ]


class Stats(C.Structure):
    _fields_ = [
        ("build_rows", C.c_int64), ("build_rows_inserted", C.c_int64), ("probe_rows", C.c_int64),
        ("out_rows", C.c_int64), ("table_bytes", C.c_int64), ("table_buckets", C.c_int64),
        ("build_kernel_ms", C.c_double), ("probe_kernel_ms", C.c_double), ("h2d_bytes", C.c_int64),
        ("d2h_bytes", C.c_int64), ("kernel_launches", C.c_int64),
        ("partition_kernel_ms", C.c_double), ("radix_probe_kernel_ms", C.c_double), ("partition_kernel_ms_sum", C.c_double),
        ("radix_probe_kernel_ms_sum", C.c_double), ("radix_timed_batches", C.c_int64), ("radix_batches", C.c_int64), ("radix_overflow_rows", C.c_int64),
        ("radix_bits", C.c_int32), ("build_partitioned", C.c_int32), ("build_handed_back_rows", C.c_int64),
        ("table_slice_bits", C.c_int32), ("build_slice_retries", C.c_int32),
        ("probe_route", C.c_int32), ("packed_key_bits", C.c_int32), ("packed_build_ms", C.c_double),
        ("heap_bytes", C.c_int64), ("heap_compactions", C.c_int64),
        ("shared_build", C.c_int32), ("dense_flushes", C.c_int32), ("shared_image_bytes", C.c_int64), ("shared_allreduce_ms", C.c_double),
        ("div_by_zero_warnings", C.c_int64),
        ("packed_lds_bits", C.c_int32), ("keyrec_digests", C.c_int32), ("side_stream_batches", C.c_int32), ("packed_lds_dup", C.c_int32),
        ("str_truncated_warnings", C.c_int64), ("str_overflow_warnings", C.c_int64),
        ("packed_interval_batches", C.c_int64),
    ]


ROUTE_DIRECT, ROUTE_RADIX_L2, ROUTE_RADIX_LDS, ROUTE_PACKED, ROUTE_KEYREC = 0, 1, 2, 3, 4


COMM_ID_BYTES = 128
KEYMODE_JOIN, KEYMODE_GROUP, KEYMODE_BROADCAST = 0, 1, 2

# tsq_ctx_set_knob (test / measurement knobs, include/tsq.h)
KNOB_DEFAULT = -(1 << 63)
(KNOB_PACKED_KEYS, KNOB_DA_MIN_BUILD_ROWS, KNOB_DA_PBITS, KNOB_PACKED_EMIT_PAIRS, KNOB_RADIX_KERNEL_L2, KNOB_LDS_NF_MAX, KNOB_RADIX_PB_MAX,
 KNOB_TABLE_LF_PERMILLE, KNOB_LDS_PROF, KNOB_DA_TRACE, KNOB_BUILD_IMAGES_CAS, KNOB_DAAGG_SIG, KNOB_DAAGG_LOG2C, KNOB_AGG_HEAP_GC_BYTES,
 KNOB_AGG_TAG_BITS, KNOB_AGG_BATCH_ROWS, KNOB_ROWCODEC_LDS_KB, KNOB_ROWCODEC_FAST_LAYOUT, KNOB_ROWCODEC_PIPELINE, KNOB_DA_PARTITION,
 KNOB_DA_NT_LOADS, KNOB_LAZY_TABLE, KNOB_DA_PAIRS_BELOW_PERMILLE, KNOB_AGG_WIDE_KEYS, KNOB_AGG_DENSE, KNOB_AGG_NARROW_CELLS, KNOB_DAAGG_PART2, KNOB_DAAGG_HOT, KNOB_KEYREC, KNOB_STREAMAGG_LANES, KNOB_XCD_ATOMICS, KNOB_DENSE_DIRECT, KNOB_DA_LDS_BUILD, KNOB_AGG_PG, KNOB_AGG_OVERLAP, KNOB_JIT_VARIANT, KNOB_HOST_OVERLAP, KNOB_HOST_NT_COPY, KNOB_KR_WG,
 KNOB_DA_PROBE_BITS, KNOB_DA_FUSED_STEP, KNOB_DA_LDS_DUP, KNOB_KEYREC_CONDS, KNOB_GROUPID_TAG_BITS, KNOB_JOIN_BATCH_TIMING,
 KNOB_ROWENC_WAVE_COPY, KNOB_LOOKUP_STRIDE, KNOB_GATHER_WAVE_COPY) = range(48)
KNOB_MVCC_WAVE_CHAIN = KNOB_XCD_ATOMICS  # the table is full: the retired id 30 (include/tsq.h)
KNOB_DA_INTERVAL, KNOB_TABLE_SIZE = 48, 49  # the first id behind TSQ_KNOB_COUNT; the table has TSQ_KNOB_TABLE_SIZE entries


# every symbol include/tsq.h declares: name -> (restype, argtypes)
P = C.c_void_p
PP = C.POINTER(C.c_void_p)
SIGNATURES = {
    "tsq_abi_version": (C.c_int32, []),
    "tsq_device_count": (C.c_int32, []),
    "tsq_last_error": (C.c_char_p, [P]),
    "tsq_ctx_create": (C.c_int32, [C.c_int32, PP]),
    "tsq_ctx_set_stream": (C.c_int32, [P, P]),
    "tsq_ctx_sync": (C.c_int32, [P]),
    "tsq_ctx_destroy": (None, [P]),
    "tsq_ctx_reserve": (C.c_int32, [P, C.c_int64]),
    "tsq_ctx_set_knob": (C.c_int32, [P, C.c_int32, C.c_int64]),
    "tsq_ctx_arena_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_dev_alloc": (C.c_int32, [P, C.c_int64, PP]),
    "tsq_dev_free": (C.c_int32, [P, P]),
    "tsq_host_alloc": (C.c_int32, [P, C.c_int64, PP]),
    "tsq_host_free": (C.c_int32, [P, P]),
    "tsq_dev_memset": (C.c_int32, [P, P, C.c_int32, C.c_int64]),
    "tsq_copy_h2d": (C.c_int32, [P, P, P, C.c_int64]),
    "tsq_copy_d2h": (C.c_int32, [P, P, P, C.c_int64]),
    "tsq_copy_d2d": (C.c_int32, [P, P, P, C.c_int64]),
    "tsq_bitmap_append": (C.c_int32, [P, P, C.c_int64, P, C.c_int64]),
    "tsq_timer_start": (C.c_int32, [P]),
    "tsq_timer_stop_ms": (C.c_int32, [P, C.POINTER(C.c_double)]),
    "tsq_gen_column": (C.c_int32, [P, C.POINTER(GenSpec), C.c_int64, P, P, P]),
    "tsq_expr_compile": (C.c_int32, [P, C.POINTER(ExprProg), C.c_int32, PP]),
    "tsq_expr_eval": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, P, C.POINTER(Col), C.POINTER(C.c_int64)]),
    "tsq_expr_eval_str": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, P, C.POINTER(Col), C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_filter_eval": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, P, P, P, C.POINTER(C.c_int64)]),
    "tsq_expr_set_jit": (C.c_int32, [P, C.c_int32]),
    "tsq_expr_jit_launches": (C.c_int64, [P]),
    "tsq_expr_jit_compile_ms": (C.c_double, [P]),
    "tsq_expr_str_warnings": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_expr_destroy": (None, [P]),
    "tsq_join_create": (C.c_int32, [P, C.POINTER(JoinCfg), PP]),
    "tsq_join_build_push": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64]),
    "tsq_join_build_finish_shared": (C.c_int32, [P, P, C.POINTER(C.c_int32)]),
    "tsq_join_set_used_columns": (C.c_int32, [P, P, C.c_int32]),
    "tsq_join_build_finish": (C.c_int32, [P]),
    "tsq_join_probe_push": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, P]),
    "tsq_join_probe_finish": (C.c_int32, [P]),
    "tsq_join_pull": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "tsq_join_set_count_only": (C.c_int32, [P, C.c_int32]),
    "tsq_join_count": (C.c_int32, [P, C.POINTER(C.c_int64)]),
    "tsq_join_checksum": (C.c_int32, [P, C.POINTER(C.c_uint64), C.POINTER(C.c_uint64)]),
    "tsq_join_set_checksum": (C.c_int32, [P, C.c_int32]),
    "tsq_join_set_ordered": (C.c_int32, [P, C.c_int32]),
    "tsq_join_set_radix": (C.c_int32, [P, C.c_int32]),
    "tsq_join_set_key_packing": (C.c_int32, [P, C.c_int32]),
    "tsq_join_cancel": (C.c_int32, [P]),
    "tsq_join_destroy": (None, [P]),
    "tsq_agg_create": (C.c_int32, [P, C.POINTER(AggCfg), PP]),
    "tsq_agg_push": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64]),
    "tsq_agg_finish": (C.c_int32, [P]),
    "tsq_agg_set_fast": (C.c_int32, [P, C.c_int32]),
    "tsq_agg_set_stream": (C.c_int32, [P, C.c_int32]),
    "tsq_agg_num_groups": (C.c_int32, [P, C.POINTER(C.c_int64)]),
    "tsq_agg_pull": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "tsq_agg_cancel": (C.c_int32, [P]),
    "tsq_agg_destroy": (None, [P]),
    "tsq_groupid_create": (C.c_int32, [P, C.POINTER(C.c_int32), C.c_int32, C.c_int64, PP]),
    "tsq_groupid_assign": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, P]),
    "tsq_groupid_count": (C.c_int32, [P, C.POINTER(C.c_int64)]),
    "tsq_groupid_keys": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.POINTER(C.c_int64)]),
    "tsq_groupid_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "tsq_groupid_cancel": (C.c_int32, [P]),
    "tsq_groupid_destroy": (None, [P]),
    "tsq_analyze_create": (C.c_int32, [P, C.POINTER(AnalyzeCfg), PP]),
    "tsq_analyze_push": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64]),
    "tsq_analyze_finish": (C.c_int32, [P]),
    "tsq_analyze_column": (C.c_int32, [P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
                                       C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_analyze_fm": (C.c_int32, [P, C.c_int32, P, C.c_int64]),
    "tsq_analyze_cm": (C.c_int32, [P, C.c_int32, P]),
    "tsq_analyze_samples_peek": (C.c_int32, [P, C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_analyze_samples": (C.c_int32, [P, C.c_int32, C.POINTER(Col), P, C.c_int64]),
    "tsq_analyze_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "tsq_analyze_cancel": (C.c_int32, [P]),
    "tsq_analyze_destroy": (None, [P]),
    "tsq_sorted_hist_create": (C.c_int32, [P, C.c_int32, C.c_int64, PP]),
    "tsq_sorted_hist_push": (C.c_int32, [P, C.POINTER(Col), C.c_int64]),
    "tsq_sorted_hist_finish": (C.c_int32, [P]),
    "tsq_sorted_hist_peek": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_sorted_hist_result": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), P, P, P, P, C.POINTER(Col), C.POINTER(Col)]),
    "tsq_sorted_hist_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_double), C.POINTER(C.c_double), C.POINTER(C.c_int64)]),
    "tsq_sorted_hist_destroy": (None, [P]),
    "tsq_agg_create_keys": (C.c_int32, [P, C.POINTER(AggCfg), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.c_int32, PP]),
    "tsq_sort_create": (C.c_int32, [P, C.POINTER(SortCfg), PP]),
    "tsq_sort_push": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64]),
    "tsq_sort_finish": (C.c_int32, [P]),
    "tsq_sort_pull": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "tsq_sort_peek": (C.c_int32, [P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "tsq_sort_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "tsq_sort_cancel": (C.c_int32, [P]),
    "tsq_sort_destroy": (None, [P]),
    "tsq_unionscan_set_slots": (C.c_int64, [C.c_int64]),
    "tsq_unionscan_create": (C.c_int32, [P, C.POINTER(UnionScanCfg), C.POINTER(C.c_int64), C.c_int64, C.POINTER(C.c_int64), C.c_int64, PP]),
    "tsq_unionscan_create_dev": (C.c_int32, [P, C.POINTER(UnionScanCfg), P, C.c_int64, P, C.c_int64, PP]),
    "tsq_unionscan_set_added": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64]),
    "tsq_unionscan_push": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64]),
    "tsq_unionscan_finish": (C.c_int32, [P]),
    "tsq_unionscan_peek": (C.c_int32, [P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "tsq_unionscan_pull": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "tsq_unionscan_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "tsq_unionscan_cancel": (C.c_int32, [P]),
    "tsq_unionscan_destroy": (None, [P]),
    "tsq_lookup_create": (C.c_int32, [P, P, C.c_int64, C.c_uint32, PP]),
    "tsq_lookup_task": (C.c_int32, [P, P, C.c_int64, C.c_uint32, C.c_int32, P, P, C.POINTER(C.c_int64)]),
    "tsq_lookup_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "tsq_lookup_cancel": (C.c_int32, [P]),
    "tsq_lookup_destroy": (None, [P]),
    "tsq_cast_create": (C.c_int32, [P, C.POINTER(CastCol), C.c_int32, C.c_uint32, C.c_uint32, PP]),
    "tsq_cast_run": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, C.POINTER(Col), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_cast_error_at": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int32)]),
    "tsq_cast_warnings": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_cast_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "tsq_cast_cancel": (C.c_int32, [P]),
    "tsq_cast_destroy": (None, [P]),
    "tsq_autoid_fill": (C.c_int32, [P, C.POINTER(Col), C.c_int64, C.c_int64, C.c_uint32, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_dupcheck_create": (C.c_int32, [P, C.POINTER(DupStream), C.c_int32, C.c_int32, P, C.c_int64, PP]),
    "tsq_dupcheck_push": (C.c_int32, [P, C.POINTER(DupKeys), C.c_int32, C.c_int64]),
    "tsq_dupcheck_match": (C.c_int32, [P, C.POINTER(DupConflict), P, P, P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_dupcheck_resolve": (C.c_int32, [P, P, C.c_int64, P, P, P, P, P, C.c_int64, C.POINTER(DupResult)]),
    "tsq_dupcheck_reset": (C.c_int32, [P]),
    "tsq_dupcheck_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "tsq_dupcheck_cancel": (C.c_int32, [P]),
    "tsq_dupcheck_destroy": (None, [P]),
    "tsq_mvcc_create": (C.c_int32, [P, C.POINTER(MvccData), PP]),
    "tsq_mvcc_scan": (C.c_int32, [P, P, P, P, C.c_int64, C.c_uint64, C.c_int32, C.c_int64, C.POINTER(MvccResult), P]),
    "tsq_mvcc_fetch": (C.c_int32, [P, P, C.c_int64, P, P, C.c_int64, P]),
    "tsq_mvcc_locked": (C.c_int32, [P, P, C.c_int64, C.POINTER(C.c_int64), P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                    C.POINTER(C.c_int32)]),
    "tsq_mvcc_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "tsq_mvcc_cancel": (C.c_int32, [P]),
    "tsq_mvcc_destroy": (None, [P]),
    "tsq_mvcc_create_rw": (C.c_int32, [P, C.POINTER(MvccData), P, P, C.c_int64, PP]),
    "tsq_mvcc_prewrite": (C.c_int32, [P, C.POINTER(MvccWriteReq), P, P, C.POINTER(MvccWriteResult), PP]),
    "tsq_mvcc_commit": (C.c_int32, [P, C.POINTER(MvccWriteReq), P, P, C.POINTER(MvccWriteResult), PP]),
    "tsq_mvcc_rollback": (C.c_int32, [P, C.POINTER(MvccWriteReq), P, P, C.POINTER(MvccWriteResult), PP]),
    "tsq_mvcc_lock_at": (C.c_int32, [P, C.c_int64, P, C.c_int64, C.POINTER(C.c_int64), P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64),
                                     C.POINTER(C.c_uint64), C.POINTER(C.c_int32)]),
    "tsq_mvcc_sizes": (C.c_int32, [P, C.POINTER(MvccStoreSizes)]),
    "tsq_mvcc_export": (C.c_int32, [P, C.POINTER(MvccArrays)]),
    "tsq_mvcc_scan_lock": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, C.c_uint64, C.POINTER(MvccLockScan)]),
    "tsq_mvcc_scan_lock_fetch": (C.c_int32, [P, P, C.c_int64, P, P, C.c_int64, P, P, P, C.c_uint32]),
    "tsq_mvcc_resolve_lock": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, P, P, C.c_int64, C.POINTER(MvccMaintResult), PP]),
    "tsq_mvcc_gc": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, C.c_uint64, C.POINTER(MvccMaintResult), PP]),
    "tsq_mvcc_delete_range": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, C.POINTER(MvccMaintResult), PP]),
    "tsq_membuf_create": (C.c_int32, [P, C.POINTER(MembufCfg), PP]),
    "tsq_membuf_push": (C.c_int32, [P, C.c_int32, P, P, C.c_int64, C.c_int64, P, P, C.c_int64, C.c_uint32, C.POINTER(C.c_int64)]),
    "tsq_membuf_finish": (C.c_int32, [P, C.POINTER(MembufResult)]),
    "tsq_membuf_request": (C.c_int32, [P, C.POINTER(MvccWriteReq)]),
    "tsq_membuf_get": (C.c_int32, [P, P, P, C.c_int64, C.c_int64, C.c_uint32, P]),
    "tsq_membuf_destroy": (None, [P]),
    "tsq_membuf_scan": (C.c_int32, [P, P, P, C.c_int64, C.c_uint32, C.c_int32, C.POINTER(MembufScanResult), P]),
    "tsq_membuf_scan_points": (C.c_int32, [P, P, P, C.c_int64, C.c_int64, C.c_uint32, C.POINTER(MembufScanResult)]),
    "tsq_membuf_fetch": (C.c_int32, [P, P, C.c_int64, P, P, C.c_int64, P]),
    "tsq_membuf_dirty": (C.c_int32, [P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_membuf_dirty_fetch": (C.c_int32, [P, P, P]),
    "tsq_unionstore_create": (C.c_int32, [P, P, P, C.c_uint64, PP]),
    "tsq_unionstore_scan": (C.c_int32, [P, P, P, C.c_int64, C.c_uint32, C.c_int32, C.c_int64, C.POINTER(UnionStoreResult), P]),
    "tsq_unionstore_get": (C.c_int32, [P, P, P, C.c_int64, C.c_int64, C.c_uint32, C.POINTER(UnionStoreResult), P]),
    "tsq_unionstore_fetch": (C.c_int32, [P, P, C.c_int64, P, P, C.c_int64, P, P]),
    "tsq_unionstore_locked": (C.c_int32, [P, P, C.c_int64, C.POINTER(C.c_int64), P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_uint64), C.POINTER(C.c_uint64),
                                          C.POINTER(C.c_int32)]),
    "tsq_unionstore_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64),
                                         C.POINTER(C.c_int32), C.POINTER(C.c_double)]),
    "tsq_unionstore_cancel": (C.c_int32, [P]),
    "tsq_unionstore_destroy": (None, [P]),
    "tsq_rows_equal": (C.c_int32, [P, C.POINTER(Col), P, C.POINTER(Col), P, C.c_int32, C.c_int64, P]),
    "tsq_rows_gather": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, P, C.c_int64, P, C.c_int64, P, C.POINTER(C.c_int64)]),
    "tsq_chunk_append": (C.c_int32, [P, C.POINTER(Col), C.c_int64, C.POINTER(C.c_int64), C.POINTER(Col), C.c_int32, C.c_int64]),
    "tsq_bytes_or": (C.c_int32, [P, P, P, C.c_int64]),
    "tsq_chunk_compact": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, P, C.POINTER(Col), C.POINTER(C.c_int64)]),
    "tsq_project_create": (C.c_int32, [P, C.POINTER(ExprProg), C.c_int32, C.POINTER(ExprProg), C.c_int32, PP]),
    "tsq_project_run": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, C.POINTER(Col), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_project_set_jit": (C.c_int32, [P, C.c_int32]),
    "tsq_project_str_warnings": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_project_stats": (C.c_int32, [P, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_double)]),
    "tsq_project_destroy": (None, [P]),
    "tsq_rows_decode": (C.c_int32, [P, P, C.c_int64, C.c_uint32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(Col), C.c_int64, C.POINTER(C.c_int64),
                                    C.POINTER(C.c_int64)]),
    "tsq_rows_decode_chunks": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, C.c_uint32, C.c_int32, C.POINTER(C.c_int32), C.POINTER(Col), C.c_int64,
                                           C.POINTER(C.c_int64)]),
    "tsq_indexkeys_decode": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, P, C.c_int64, P, C.c_uint32, C.c_int32, C.POINTER(C.c_int32), C.c_int32, C.POINTER(Col),
                                         C.POINTER(C.c_int64)]),
    "tsq_chunk_encode": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int64, P, C.c_int64, C.c_uint32, C.POINTER(C.c_int64)]),
    "tsq_chunk_decode_peek": (C.c_int32, [P, P, C.c_int64, C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.c_int64, C.POINTER(C.c_int64),
                                          C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_chunk_decode": (C.c_int32, [P, P, C.c_int64, C.c_uint32, C.POINTER(C.c_int32), C.c_int32, C.c_int64, C.c_int64, C.POINTER(Col),
                                     C.POINTER(C.c_int64), C.POINTER(C.c_int64)]),
    "tsq_rowcodec_decode": (C.c_int32, [P, P, C.c_int64, P, P, C.c_int64, C.c_uint32, C.c_int32, C.POINTER(RowcodecCol), C.POINTER(Col),
                                        C.POINTER(C.c_int64)]),
    "tsq_rows_encode": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.POINTER(C.c_uint32), C.c_int64, P, C.c_int64, C.c_uint32, P, C.POINTER(C.c_int64)]),
    "tsq_rowkeys_decode": (C.c_int32, [P, P, C.c_int64, P, C.c_int64, C.c_uint32, P, P, C.POINTER(C.c_int64)]),
    "tsq_rowkeys_encode": (C.c_int32, [P, C.c_int64, P, C.c_int64, C.c_uint32, P]),
    "tsq_rowcodec_encode": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.POINTER(C.c_int64), C.POINTER(C.c_uint32), C.c_int64, P, C.c_int64, C.c_uint32, P,
                                        C.POINTER(C.c_int64)]),
    "tsq_indexkeys_encode": (C.c_int32, [P, C.c_int64, C.c_int64, C.c_uint32, C.POINTER(Col), C.c_int32, C.POINTER(C.c_int32), P, P, C.c_int64, C.c_uint32,
                                         P, C.c_int64, P, P, P, P, C.POINTER(C.c_int64)]),
    "tsq_radix_split": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32,
                                    C.POINTER(Col), C.POINTER(C.c_int64)]),
    "tsq_comm_unique_id": (C.c_int32, [P]),
    "tsq_comm_create": (C.c_int32, [P, C.c_int32, C.c_int32, P, PP]),
    "tsq_comm_destroy": (None, [P]),
    "tsq_comm_allreduce_i64": (C.c_int32, [P, C.POINTER(C.c_int64), C.c_int32, C.c_int32]),
    "tsq_comm_allreduce_f64": (C.c_int32, [P, C.POINTER(C.c_double), C.c_int32, C.c_int32]),
    "tsq_comm_info": (C.c_int32, [P, C.POINTER(C.c_int32), C.POINTER(C.c_int32), C.POINTER(C.c_int32)]),
    "tsq_comm_barrier": (C.c_int32, [P]),
    "tsq_redistribute": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32, C.POINTER(Col), C.POINTER(C.c_int64)]),
    "tsq_redistribute_wait": (C.c_int32, [P, C.c_int32]),
    "tsq_redistribute_prepare": (C.c_int32, [P, C.POINTER(Col), C.c_int32, C.c_int32, C.c_int32, C.c_int64, C.c_int32]),
    "tsq_redistribute_counts": (C.c_int32, [P, C.POINTER(C.c_int32), C.c_int32]),
    "tsq_redistribute_issue": (C.c_int32, [P, C.c_int32, C.POINTER(Col), C.c_int32, C.POINTER(C.c_int64)]),
    "tsq_join_peek": (C.c_int32, [P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "tsq_agg_peek": (C.c_int32, [P, C.c_int64, C.POINTER(C.c_int64), C.POINTER(C.c_int64), C.c_int32]),
    "tsq_join_stats": (C.c_int32, [P, C.POINTER(Stats)]),
    "tsq_agg_stats": (C.c_int32, [P, C.POINTER(Stats)]),
}
