/*
 * tsq.h — C-ABI of libtsq: the MI355X (gfx950) hot path for TinySQL's chunked operators.
 *
 * This is the drop-in boundary: plain C, plain pointers and sizes, no C++/torch types.
 * A cgo shim inside TinySQL's package `executor` binds exactly these symbols
 * (see INTEGRATION.md).  Every entry point cites the reference interface it replaces
 * (paths relative to the TinySQL tree).
 *
 * Conventions
 *   - every function returns a tsq_status (int32_t); 0 == TSQ_OK.  Nothing aborts/exits.
 *   - tsq_last_error(handle) returns a human readable message for the last failure on
 *     that handle (or the last creation failure when handle == NULL).
 *   - handles are NOT thread-affine (executor/join.go:207, aggregate.go:512 call Next from
 *     background goroutines): every entry point sets its own device and uses the handle's
 *     own HIP stream; one caller at a time per handle, except tsq_*_cancel which may be
 *     called from any thread at any time.
 *   - host pointers passed in are only read/written for the duration of the call
 *     (cgo pointer rule); nothing is retained.
 *   - a column (tsq_col) mirrors util/chunk/column.go:28-34: fixed-width little-endian
 *     data, null bitmap with bit==1 meaning NOT NULL, LSB first (column.go:89-92);
 *     null_bitmap == NULL means "no NULLs".
 */
#ifndef TSQ_H
#define TSQ_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#define TSQ_ABI_VERSION 10
/* (round 15 appended tsq_stats.packed_interval_batches and the knob id 48 without a new number: rebuild hosts against this header) */

/* ---------------------------------------------------------------- status codes */
typedef int32_t tsq_status;
enum {
    TSQ_OK = 0,
    TSQ_ERR_INVALID = 1,          /* bad argument / bad state (maps to a Go errors.New)          */
    TSQ_ERR_UNSUPPORTED = 2,      /* plan not eligible: caller must fall back to the Go operator */
    TSQ_ERR_OOM_DEVICE = 3,
    TSQ_ERR_HIP = 4,
    TSQ_ERR_OVERFLOW_BIGINT = 5,  /* types.ErrOverflow "BIGINT"           (types/overflow.go:33-40) */
    TSQ_ERR_OVERFLOW_BIGINT_UNSIGNED = 6, /* types.ErrOverflow "BIGINT UNSIGNED"                  */
    TSQ_ERR_OVERFLOW_DOUBLE = 7,  /* types.ErrOverflow "DOUBLE" (builtin_arithmetic_vec.go:51)     */
    TSQ_ERR_CANCELLED = 8,        /* tsq_*_cancel was called (executor.go:158 kill flag)           */
    TSQ_ERR_NO_DEVICE = 9,        /* no HIP device visible: the product path never falls back     */
    TSQ_ERR_DIV_BY_ZERO = 10,     /* only in strict INSERT/DELETE mode (expression/errors.go:65-77)*/
    TSQ_ERR_TRUNCATED_WRONG_VALUE = 11, /* ABI 8: types.ErrTruncatedWrongVal of a string filter value when truncation is an error */
    /* tsq_cast_run / tsq_autoid_fill (additions to ABI 10: no existing value changes) */
    TSQ_ERR_DATA_TOO_LONG = 12,   /* types.ErrDataTooLong (types/datum.go:620-624)                                       */
    TSQ_ERR_OUT_OF_RANGE = 13,    /* types.ErrOverflow of a cast (types/convert.go:93-174); tsq_cast_error_at names the column */
    TSQ_ERR_BAD_NULL = 14,        /* table.ErrColumnCantNull (table/column.go:281-299)                                    */
    TSQ_ERR_BAD_UTF8 = 15,        /* table.ErrTruncatedWrongValueForField of handleWrongUtf8Value (table/column.go:107-138) */
    /* tsq_dupcheck_match (addition to ABI 10) */
    TSQ_ERR_KEY_EXISTS = 16,      /* kv.ErrKeyExists "Duplicate entry" (kv/error.go, executor/batch_checker.go:114,138-146)          */
    /* tsq_mvcc_scan (addition to ABI 10) */
    TSQ_ERR_LOCKED = 17           /* mocktikv.ErrLocked: a read met another transaction's lock (mvcc.go:187-207); tsq_mvcc_locked names it */
};

/* ---------------------------------------------------------------- column ABI */
/* element types (types/eval_type.go:21-28 has only Int/Real/String eval types) */
enum {
    TSQ_I64 = 0,   /* bigint and narrower ints, stored as 8 bytes (util/chunk/codec.go:171-181) */
    TSQ_U64 = 1,   /* same 8 bytes, UNSIGNED flag set in FieldType.Flag                         */
    TSQ_F32 = 2,   /* float, 4 bytes                                                            */
    TSQ_F64 = 3,   /* double, 8 bytes                                                           */
    TSQ_BYTES = 4  /* var-len (offsets[n+1] + data), binary collation: expression inputs (string builtins), join payload
                      and join keys, group keys and FIRST_ROW / MAX / MIN / COUNT arguments of the aggregate */
};

/* tsq_col.flags */
#define TSQ_COL_DEVICE 1u /* data/null_bitmap/offsets are device (HBM) pointers */
#define TSQ_COL_RETAIN 4u /* ABI 7, an INPUT column of tsq_join_build_push: the operator may KEEP this device buffer as its build-side storage
                           * instead of copying the rows — what the reference does with the chunks it is handed (hash_table.go:146-169 PutChunk ->
                           * chunk.List.Add keeps the chunk, util/chunk/list.go:96-110).  The caller leaves the buffer (and its null bitmap) unchanged and
                           * allocated until tsq_join_destroy.  Honoured for the FIRST push of a build side when every column is a fixed-width
                           * TSQ_COL_DEVICE | TSQ_COL_RETAIN column whose buffers are whole tsq_dev_alloc blocks; otherwise the rows are copied as always
                           * (later pushes copy the retained rows into the operator's own storage first). */
#define TSQ_COL_BORROW 2u /* an OUTPUT column of a pull (tsq_join_pull; device-resident pulls, and since round 6 host pulls too — the pointers then
                             lead into the operator's PINNED result batch, which the D2H copies filled): instead of copying into the caller's buffers the
                             operator hands out pointers into its own result batch — data / null_bitmap are SET by the call (null_bitmap =
                             NULL when the column holds no NULL) and stay valid until the next pull, peek, finish or destroy on the handle (tsq_join_peek
                             releases fully consumed result batches too).
                             The device-chunk hand-off between GPU operators (Chunk.SwapColumns, util/chunk/chunk.go:231-235, is the
                             same idea: ownership of the buffers moves, no row is copied).  Fixed-width columns only. */

/* mirrors util/chunk/column.go:28-34 */
typedef struct tsq_col {
    void*    data;         /* fixed: length*elem_size bytes, native little endian                */
    uint8_t* null_bitmap;  /* (length+7)/8 bytes, bit=1 => NOT NULL; NULL => column has no NULL */
    int64_t* offsets;      /* var-len only (length+1 entries, first 0); NULL for fixed           */
    int64_t  length;       /* rows                                                               */
    int32_t  elem_size;    /* 4, 8, or -1 for var-len                                            */
    int32_t  type;         /* TSQ_I64 ...                                                        */
    uint32_t flags;        /* TSQ_COL_DEVICE                                                     */
    uint32_t reserved;
} tsq_col;

/* ---------------------------------------------------------------- misc / context */
typedef struct tsq_ctx tsq_ctx;

int32_t     tsq_abi_version(void);
int32_t     tsq_device_count(void);                 /* 0 when no GPU is visible */
const char* tsq_last_error(const void* handle);     /* handle may be ctx/join/agg/expr or NULL */

/* One context per (process, device).  All operators created from it share its stream. */
tsq_status tsq_ctx_create(int32_t device, tsq_ctx** out);
/* Use an externally owned hipStream_t (e.g. torch's current stream) instead of the ctx's own. */
tsq_status tsq_ctx_set_stream(tsq_ctx* ctx, void* hip_stream);
tsq_status tsq_ctx_sync(tsq_ctx* ctx);
void       tsq_ctx_destroy(tsq_ctx* ctx);
/* Reserve `bytes` of HBM as the context's ARENA: the buffers of every operator created from the context (hash tables, partition
 * stores, result batches, tsq_dev_alloc blocks) are carved from it, so the first query of a session does not pay hipMalloc's
 * first touch (~35 ms per GB: 310 ms for a 1e8-row build side, 2.7 ms once the memory is there).  Call it when the host process
 * creates the context (the reference recycles its chunks through outerChkResourceCh / joinChkResourceCh instead of allocating
 * per batch, executor/join.go:54-56,169-171, and a Go process keeps its heap across queries); a request the arena cannot hold
 * falls through to hipMalloc.  bytes = 0 gives the arena back; not allowed
 * while operators hold buffers of it.  tsq_ctx_arena_stats: slab size, bytes in use, high-water mark. */
tsq_status tsq_ctx_reserve(tsq_ctx* ctx, int64_t bytes);
/* TEST AND MEASUREMENT KNOBS.  A host never calls this: every knob defaults to what the library was measured and tested
 * with.  The parity tests use them to force the rarely taken variants (a heap compaction after every batch, truncated group
 * tags, the un-pipelined row decoder ...), tools/ and bench.py to A/B kernel variants on one box.  They replace the
 * environment variables earlier rounds read inside the product code.  value = TSQ_KNOB_DEFAULT restores the default.
 * A knob is read when the operator takes the decision it steers (usually at its first batch). */
#define TSQ_KNOB_DEFAULT INT64_MIN
enum {
    TSQ_KNOB_PACKED_KEYS = 0,        /* 0: no packed-key routes (join and aggregate) */
    TSQ_KNOB_DA_MIN_BUILD_ROWS = 1,  /* build rows from which AUTO tries the packed routes (default 1 Mi) */
    TSQ_KNOB_DA_PBITS = 2,           /* log2(partitions) of the packed routes (default: min(11, b - 10)) */
    TSQ_KNOB_PACKED_EMIT_PAIRS = 3,  /* 1: AUTO may take the pairs variant of the materialising packed route (K4d) */
    TSQ_KNOB_RADIX_KERNEL_L2 = 4,    /* 1: the 64-bit radix probe keeps round 1's L2 route */
    TSQ_KNOB_LDS_NF_MAX = 5,         /* cap on the table slices per LDS image (forces S > 1 on small tables) */
    TSQ_KNOB_RADIX_PB_MAX = 6,       /* cap on log2(partitions) of the 64-bit radix probe */
    TSQ_KNOB_TABLE_LF_PERMILLE = 7,  /* load factor of a sliced join table, in 1/1000 (default 750) */
    TSQ_KNOB_LDS_PROF = 8,           /* 1: per-phase shader cycles of the LDS probe on stderr (synchronises) */
    TSQ_KNOB_DA_TRACE = 9,           /* 1: host time points of the travelling-columns route on stderr */
    TSQ_KNOB_BUILD_IMAGES_CAS = 10,  /* 1: the first (compare-and-swap) slice-image kernel of the partitioned build */
    TSQ_KNOB_DAAGG_SIG = 11,         /* 0: no plan-specialised instantiations of k_agg_da; 1: SUM + COUNT(*) plans; 2 (default since round 6): also count and sum of 2-byte cells in one LDS word */
    TSQ_KNOB_DAAGG_LOG2C = 12,       /* log2(cells per LDS table) of the packed aggregate, 9..12 */
    TSQ_KNOB_AGG_HEAP_GC_BYTES = 13, /* string-heap size from which the aggregate compacts between batches (default 256 MiB) */
    TSQ_KNOB_AGG_TAG_BITS = 14,      /* truncate the 64-bit group tag of a several-column GROUP BY (collision tests) */
    TSQ_KNOB_AGG_BATCH_ROWS = 15,    /* device batch of host-pushed aggregate input (default 4 Mi rows) */
    TSQ_KNOB_ROWCODEC_LDS_KB = 16,   /* LDS tile of the stored-row decoder */
    TSQ_KNOB_ROWCODEC_FAST_LAYOUT = 17, /* 0: every wave takes the per-row column search */
    TSQ_KNOB_ROWCODEC_PIPELINE = 18, /* 0: the un-pipelined decoder kernel */
    TSQ_KNOB_DA_PARTITION = 19,      /* packed partition kernel: 0 = default per entry width and batch size, 1 = one 1024-thread workgroup per CU of the un-pipelined kernel, 2 = two of 512, 3 = two of 512 with the next tile's key loads in flight (2-byte entries without bitmaps / flags / several columns; the others run as with 2), 4 = as 3 on a tile of 32 Ki keys: one 1024-thread workgroup per CU (2-byte entries; profiles/r13_step_ab.txt) — what the default takes for batches with at least one such tile per CU, while 3 keeps the 16 Ki-key tile for every batch */
    TSQ_KNOB_DA_NT_LOADS = 20,       /* 0: plain instead of non-temporal key loads in k_da_partition2 */
    TSQ_KNOB_LAZY_TABLE = 21,        /* 0: tsq_join_build_finish always builds the 64-bit table (default: a build side the packed routes are likely to
                                        serve leaves it to the first probe batch that needs it) */
    TSQ_KNOB_DA_PAIRS_BELOW_PERMILLE = 22, /* AUTO: a probe batch whose sampled hit ratio lies below this (in 1/1000, default 350) takes the pairs
                                        variant of the materialising packed route (K4d) instead of the travelling columns (K5f + K4e) */
    TSQ_KNOB_AGG_WIDE_KEYS = 23,     /* 0: several integer group-key columns never become one 64-bit composite key (the several-column upsert keeps them) */
    TSQ_KNOB_AGG_DENSE = 24,         /* 0: the one-key packed aggregate appends partial groups after every batch instead of folding its LDS tables into the dense state; v > 1 (tests): the state is emptied into the table before more than v rows went into it (default 2^31) */
    TSQ_KNOB_AGG_NARROW_CELLS = 25,  /* 0: the argument column of the packed aggregate always travels as 8-byte cells */
    TSQ_KNOB_DAAGG_PART2 = 26,       /* partition kernel of the packed aggregate with a dense state: 0 = 1024 threads, one workgroup per CU; 1 = two 512-thread workgroups per CU for narrow argument cells (default); 2 = for 8-byte cells too */
    TSQ_KNOB_DAAGG_HOT = 27,         /* 0: the packed aggregate does not sample the batch for hot keys (their rows then travel through the partitioned store and its overflow store) */
    TSQ_KNOB_KEYREC = 28,            /* 0: joins on several key columns / string keys never take the key-record route (csrc/tsq_keyrec.h), aggregates never the dictionary of group keys (csrc/tsq_keydict.h); 2: the dictionary's scatter pass writes separate arrays instead of 64-byte slots; 3 (tests): the digest of a long string cell carries its length only, so that every two cells of one length are candidates and the byte comparison decides */
    TSQ_KNOB_STREAMAGG_LANES = 29,   /* 0: StreamAggExec always reduces every 64-row step across the lanes (k_sa_update) instead of keeping per-lane partial results of the open run (k_sa_update_lanes) */
    TSQ_KNOB_XCD_ATOMICS = 30,       /* retired in round 6 (was: workgroup-scope cursor atomics, an A/B that measured equal); setting it has no effect */
    TSQ_KNOB_DENSE_DIRECT = 31,      /* 0: the packed aggregate's dense state always leaves through partial groups and the hash table, also when the table is empty (k_dense_finalize off) */
    TSQ_KNOB_DA_LDS_BUILD = 32,      /* 0: the materialising packed join never keeps a partition's build rows in LDS (csrc/tsq_damat.h): unique build sides take the sorted-build-columns variant of round 4 like the others; 2 .. 5 (tests): the second partition level splits 1 / 2 / 4 / 8 ways whatever the build side's size */
    TSQ_KNOB_AGG_PG = 33,            /* 0: an aggregate with about as many groups as rows never keeps its groups in partitioned LDS-sized sub-tables (csrc/tsq_aggfast.h K7p): the row upsert serves it; v >= 2 (tests): the mode is taken whatever the estimate, with 2^(v - 2) sub-tables */
    TSQ_KNOB_AGG_OVERLAP = 34,       /* default 0: the packed aggregate with a dense state runs every batch on one stream (partition pass, then k_agg_da); 1: k_agg_da / k_daagg_ovf of a batch run on a side stream beside the partition pass of the next batch (two partitioned stores) for batches of 2^24 rows or more — an A/B that measured SLOWER (C3 7.0 -> 10.1 ms, profiles/r06_ab_measurements.txt); v >= 2 (tests): for batches of v rows or more */
    TSQ_KNOB_JIT_VARIANT = 35,       /* A/B bits of the hiprtc-specialised projection kernel (jit_expr), default 391 = 7 | 128 | 256 (measured 0.525 -> 0.453 ms per 1e8 rows of (a+b)*3-a against 0, the filter a<b AND c>0.5 0.463 -> 0.429 ms, profiles/r06_jit_sweep.txt): 1 = non-temporal loads of the input cells, 2 = non-temporal stores of the result, 4 = whole-wave coalesced 16-byte accesses (a lane takes rows 2 l, 2 l + 1 of each 128-row half of a 256-row step instead of four consecutive rows), 8 = two steps' loads in flight; bits 4-6: workgroups per CU = 8 (0), 4, 16, 32, 2; 128 = jit_filter reads its 8-byte cells with non-temporal loads, 256 = and writes the selected byte with a non-temporal store */
    TSQ_KNOB_HOST_OVERLAP = 36,      /* bits of the pipelining of a join fed with HOST chunks (default 3; 0 = rounds 1-5: one stream, every result batch copied to pinned memory and waited for): 1 = the D2H copies run on the operator's copy stream beside the staging, H2D and kernels of the next batch, a flush waits for its H2D copies only, and tsq_join_pull answers "no rows yet" while the front batch is still on its way and the probe side is not finished; 2 = the H2D copies of staged probe rows are queued every 256 Ki rows while the caller still pushes (a software prefetch of the next pull's first lines was measured without effect and removed) */
    TSQ_KNOB_HOST_NT_COPY = 37,      /* 0: host chunks enter the pinned staging buffers through memcpy instead of non-temporal stores (process-wide) */
    TSQ_KNOB_KR_WG = 38,             /* workgroups (contiguous row chunks) of the key-record hist / scatter passes, 8..256 (default 256): fewer workgroups keep fewer partition lines open at once (A/B, profiles/r06_keyrec_ab.txt) */
    TSQ_KNOB_DA_PROBE_BITS = 39,     /* COUNT(*) probe of a unique build side with byte cells (2-byte entries): 0 = it reads the 64 KB byte images; n >= 1 = their bit form (8 KB per partition, derived once per build side by k_da_bytes_to_bits) with n probe workgroups per CU */
    TSQ_KNOB_DA_FUSED_STEP = 40,     /* COUNT(*) step of the packed route (da_probe): 1 (default) = two launches — the probe kernel counts the overflow list and leaves the cursors clean for the next batch; 0 = memsets + partition + probe + overflow kernel, as before */
    TSQ_KNOB_DA_LDS_DUP = 41,        /* the materialising packed join keeps the build rows of a build side WITH duplicate keys (<= 255 rows per key) in LDS (csrc/tsq_damat_dup.h): 0 = never (the sorted-build-columns variant keeps them); 1 (default) = AUTO: when the build side has at least TSQ_DM_DUP_MIN_BUILD_ROWS rows (measured, never below 65 536: profiles/r09_lds_dup_ab.txt); v >= 2 (tests, A/B) = when it has at least v rows.  TSQ_KNOB_DA_LDS_BUILD = 0 switches both LDS variants off, its values 2 .. 5 force S for both */
    TSQ_KNOB_KEYREC_CONDS = 42,      /* a join on several key columns / string keys WITH OtherConditions: 0 = it never takes the key-record route (the direct route evaluates the conditions, as before round 10); 1 (default) = AUTO: it takes the route at the route's own gate (65 536 rows on both sides, or radix FORCE) and the probe kernel evaluates the conditions on every key-equal candidate (csrc/tsq_keyrec.h: k_kr_probe<VERIFY, COND>) — measured faster than the direct route at every swept size, 2^16 .. 1e7 rows per side (profiles/r10_keyrec_conds_ab.txt) */
    TSQ_KNOB_COUNT = 48
};
/* Ids behind the 48 of the table above: the table itself has TSQ_KNOB_TABLE_SIZE entries, tsq_ctx_set_knob takes the ids below that. */
/* id 48: COUNT(*) against a build side that fills its key interval — unique keys, as many usable rows as kmax - kmin + 1 (tsq_da_is_interval, csrc/tsq_dapack.h; byte cells, one key column) — is one range test per probe key (k_da_interval_count) instead of partition + probe: 1 (default) = when key packing is in AUTO mode; 0 = never (the partitioned kernels, for A/B); 2 = also under tsq_join_set_key_packing(FORCE) (tests on small build sides) */
#define TSQ_KNOB_DA_INTERVAL (TSQ_KNOB_COUNT + 0)
#define TSQ_KNOB_TABLE_SIZE (TSQ_KNOB_COUNT + 1)
/* one more id of the same table (the table has TSQ_KNOB_COUNT entries; 43..47 were free): keep only this many bits of a row's hash in tsq_groupid — for BOTH the slot index and the tag — so that distinct keys meet in one slot with one tag and the cell comparison decides (collision tests) */
#define TSQ_KNOB_GROUPID_TAG_BITS 43
/* id 44 of the same table: which partitioned probe batches of a join handle record HIP events around their kernels (start, behind the partition pass, end — a marker packet each on the stream).  N > 0: batch b is timed iff b % N == N - 1; 0: never; 1: every batch (as before round 13); default 4.  tsq_join_stats sums the timed batches among the 32 most recent (radix_timed_batches of them); probe_kernel_ms is the last timed batch */
#define TSQ_KNOB_JOIN_BATCH_TIMING 44
/* id 45 of the same table: tsq_rowcodec_encode / tsq_indexkeys_encode let the 64 lanes of a wave copy a var-len cell of at least this many bytes (consecutive lanes, consecutive bytes) instead of the lane that owns the row; <= 0: never; default 64 (profiles/write_path_ab.txt) */
#define TSQ_KNOB_ROWENC_WAVE_COPY 45
/* id 46 of the same table: log2 of the sampling stride of the search index tsq_lookup_create builds over a table's handles (every 2^s-th handle, every 2^s-th of those, ... until the top level has at most 1024 entries); 0: no index, the plain lower bound over the whole table; read at create; default 4, the fastest stride of the sweep over 1e8 handles (profiles/index_lookup_ab.txt) */
#define TSQ_KNOB_LOOKUP_STRIDE 46
/* id 47 of the same table: tsq_rows_gather lets the 64 lanes of a wave copy a row of at least this many bytes (consecutive lanes, consecutive bytes) instead of the lane that owns the row; <= 0: never; default 64 (A/B over never, 8, 64, 256: profiles/index_lookup_ab.txt) */
#define TSQ_KNOB_GATHER_WAVE_COPY 47
/* the table is full: this one takes the id of the retired TSQ_KNOB_XCD_ATOMICS (30, without effect since round 6).  tsq_mvcc_scan lets the 64 lanes of a wave walk a key's version chain of at least this many versions, 64 versions per step, instead of the lane that owns the key; <= 0: never; default 64, one wave step: 16 .. 4096 measure equal on chains of 1..5 versions and on a key with 1e6 versions, 4 costs 3.7 x on the short chains, never 10 x on the long one (profiles/mvcc_scan_ab.txt) */
#define TSQ_KNOB_MVCC_WAVE_CHAIN TSQ_KNOB_XCD_ATOMICS
tsq_status tsq_ctx_set_knob(tsq_ctx* ctx, int32_t knob, int64_t value);
tsq_status tsq_ctx_arena_stats(tsq_ctx* ctx, int64_t* size_out, int64_t* used_out, int64_t* peak_out);

/* Device memory + copies for harnesses that keep tables resident in HBM (bench, multi-GPU). */
tsq_status tsq_dev_alloc(tsq_ctx* ctx, int64_t bytes, void** out);
tsq_status tsq_dev_free(tsq_ctx* ctx, void* p);
tsq_status tsq_dev_memset(tsq_ctx* ctx, void* p, int32_t byte, int64_t bytes);
/* Pinned host memory (ABI 6) for the chunks a host pushes or pulls and for tsq_copy_h2d / tsq_copy_d2h: the DMA engines read and write
 * it directly, a pageable Go / numpy buffer goes through a bounce buffer at a fraction of the link rate (BASELINE north star: "chunk.Column
 * batches pinned and DMA'd to HBM").  The cgo shim keeps its chunk.Column data in such blocks; freed blocks return to
 * a process-wide pool. */
tsq_status tsq_host_alloc(tsq_ctx* ctx, int64_t bytes, void** out);
tsq_status tsq_host_free(tsq_ctx* ctx, void* p);
tsq_status tsq_copy_h2d(tsq_ctx* ctx, void* dst_dev, const void* src_host, int64_t bytes);
tsq_status tsq_copy_d2h(tsq_ctx* ctx, void* dst_host, const void* src_dev, int64_t bytes);
/* device to device, queued on the context's stream (not synchronised): an operator's output batch kept beyond its next Next() */
tsq_status tsq_copy_d2d(tsq_ctx* ctx, void* dst_dev, const void* src_dev, int64_t bytes);
/* rows [dst_rows, dst_rows + n) of a device null bitmap := the first n bits of src_bitmap (device; NULL: n NOT-NULL bits) — the bit
 * offset is arbitrary (Column.appendNullBitmap, util/chunk/column.go; chunk.Decoder.decodeColumn's shift-and-or, codec.go:325-343).
 * Queued on the context's stream.  The destination must hold (dst_rows + n + 7) / 8 + 8 bytes. */
tsq_status tsq_bitmap_append(tsq_ctx* ctx, uint8_t* dst_bitmap, int64_t dst_rows, const uint8_t* src_bitmap, int64_t n);

/* Timing helper: HIP events recorded on the ctx stream (bench.py's roofline leg). */
tsq_status tsq_timer_start(tsq_ctx* ctx);
tsq_status tsq_timer_stop_ms(tsq_ctx* ctx, double* ms_out); /* synchronises the stop event */

/* ---------------------------------------------------------------- synthetic tables
 * Counter-based generator, identical on host (oracle) and device:
 *   r(i,c) = splitmix64(seed ^ (table<<56) ^ (c<<48) ^ i)
 * Replaces the reference's mockDataSource generators (executor/benchmark_test.go:50-177). */
enum {
    TSQ_GEN_SEQ = 0,        /* v = start + i                                   (benchmark_test.go:396-407) */
    TSQ_GEN_AFFINE = 1,     /* v = (a*i + b) mod m : bijection on [0,m) when gcd(a,m)=1, m < 2^31        */
    TSQ_GEN_RAND_MOD = 2,   /* v = r(i,c) mod m                                                           */
    TSQ_GEN_RAND_F64 = 3,   /* v = (r(i,c)>>11) * 2^-53 in [0,1)  (rand.Float64, benchmark_test.go:118)   */
    TSQ_GEN_HASH_OF_COL = 4,/* v = splitmix64(src[i] ^ b): payload that is a function of another column  */
    TSQ_GEN_ZIPF_OCT = 5    /* skewed keys with the s = 1 harmonic envelope, piecewise constant per octave: an octave e is drawn uniformly
                               from [0, a), then a value uniformly from [2^e, 2^(e+1)); v = (that - 1) mod m.  P(v) ~ 1 / (a 2^floor(log2(v+1))):
                               key 0 takes 1 / a of the rows (C3 with Zipf s = 1.0 keys)                */
};
typedef struct tsq_gen_spec {
    int32_t  kind;
    int32_t  table;      /* t */
    int32_t  col;        /* c */
    int32_t  null_pct;   /* 0..100: row is NULL iff r(i,7) % 100 < null_pct */
    uint64_t seed;
    int64_t  start;      /* SEQ start / global row offset i0 for all kinds (row index = i0 + i) */
    uint64_t a, b, m;    /* AFFINE / RAND_MOD parameters */
} tsq_gen_spec;
/* dst/null_bitmap/src are device pointers; null_bitmap may be NULL when null_pct == 0. */
tsq_status tsq_gen_column(tsq_ctx* ctx, const tsq_gen_spec* spec, int64_t nrows,
                          void* dst, uint8_t* null_bitmap, const void* src);

/* ---------------------------------------------------------------- vectorized expressions
 * Replaces expression.VecExpr / VecEval{Int,Real} (expression/expression.go:43-55,329-341),
 * VectorizedFilter (chunk_executor.go:196-245) and EvaluatorSuite.Run (evaluator.go:121-133):
 * the Go side flattens an expression tree to postfix bytecode; ONE fused kernel evaluates the
 * whole tree per row instead of one pass per node.  Each opcode is one reference signature. */
enum {
    /* leaves */
    TSQ_OP_COL_INT = 1,     /* arg = column index            (expression/column.go:56-75)          */
    TSQ_OP_COL_REAL = 2,    /* arg = column index; F32 widened (column.go:81-104)                  */
    TSQ_OP_CONST_INT = 3,   /* arg = const index             (constant.go:76-88, vectorized.go:23) */
    TSQ_OP_CONST_REAL = 4,
    TSQ_OP_CONST_NULL_INT = 5,
    TSQ_OP_CONST_NULL_REAL = 6,
    /* arithmetic (builtin_arithmetic_vec.go) */
    TSQ_OP_PLUS_REAL = 10,  /* :275 */
    TSQ_OP_MINUS_REAL = 11, /* :62  */
    TSQ_OP_MUL_REAL = 12,   /* :29  */
    TSQ_OP_DIV_REAL = 13,   /* :348 */
    TSQ_OP_PLUS_INT = 14,   /* :389 (+plusUU/US/SU/SS :428-495), flags = unsigned bits           */
    TSQ_OP_MINUS_INT = 15,  /* :95  (+minusFUU..SS :142-271), flags = unsigned bits|FORCE_SIGNED  */
    TSQ_OP_MUL_INT = 16,    /* :308 */
    TSQ_OP_MUL_INT_UNSIGNED = 17, /* :501 */
    /* compare (builtin_compare_vec.go:26-292, builtin_compare_vec_generated.go) */
    TSQ_OP_LT_INT = 20, TSQ_OP_LE_INT = 21, TSQ_OP_GT_INT = 22, TSQ_OP_GE_INT = 23,
    TSQ_OP_EQ_INT = 24, TSQ_OP_NE_INT = 25,
    TSQ_OP_LT_REAL = 26, TSQ_OP_LE_REAL = 27, TSQ_OP_GT_REAL = 28, TSQ_OP_GE_REAL = 29,
    TSQ_OP_EQ_REAL = 30, TSQ_OP_NE_REAL = 31,
    /* logic / unary (builtin_op_vec.go) */
    TSQ_OP_LOGIC_AND = 40,  /* :173 */
    TSQ_OP_LOGIC_OR = 41,   /* :29  */
    TSQ_OP_NOT_INT = 42,    /* :249 */
    TSQ_OP_NOT_REAL = 43,   /* :141 */
    TSQ_OP_NEG_INT = 44,    /* :221, flags bit0 = arg unsigned */
    TSQ_OP_NEG_REAL = 45,   /* :74  */
    TSQ_OP_ISNULL_INT = 46, /* :92  */
    TSQ_OP_ISNULL_REAL = 47,/* :113 */
    /* control (builtin_control_vec_generated.go) */
    TSQ_OP_IFNULL_INT = 50, /* :23  */
    TSQ_OP_IFNULL_REAL = 51,/* :52  */
    TSQ_OP_IF_INT = 52,     /* :117 (cond is Int; value args Int)  */
    TSQ_OP_IF_REAL = 53,    /* :163 */
    /* IN (builtin_other_vec_generated.go); arg = number of list items n (stack: x, v1..vn) */
    TSQ_OP_IN_INT = 60,     /* :24, flags bit0 = x unsigned; unsigned-ness of item j in in_unsigned_mask bit j */
    TSQ_OP_IN_REAL = 61,    /* :151 */
    /* strings (types.EvalType ETString), binary collation: types.CompareString = bytes.Compare.  A string VALUE on the evaluation
     * stack is a reference (source column or the program's constant pool, byte offset, length): no bytes are copied. */
    TSQ_OP_COL_STR = 70,        /* arg = column index (TSQ_BYTES)        (expression/column.go:106-129)              */
    TSQ_OP_CONST_STR = 71,      /* arg = const index: consts[arg] = (offset into str_pool << 32) | length            */
    TSQ_OP_CONST_NULL_STR = 72,
    TSQ_OP_LT_STR = 73, TSQ_OP_LE_STR = 74, TSQ_OP_GT_STR = 75, TSQ_OP_GE_STR = 76,  /* builtin_compare_vec_generated.go:65,147,229,311 */
    TSQ_OP_EQ_STR = 77, TSQ_OP_NE_STR = 78,                                          /* :393, :475                                      */
    TSQ_OP_STRCMP = 79,         /* builtin_string_vec.go:52  -> -1 / 0 / 1                                          */
    TSQ_OP_LENGTH = 80,         /* builtin_string_vec.go:89  -> bytes                                               */
    TSQ_OP_ISNULL_STR = 81,     /* builtin_string_vec.go:21 (builtinStringIsNullSig)                                */
    TSQ_OP_IFNULL_STR = 82,     /* builtin_control_vec_generated.go:81                                              */
    TSQ_OP_IF_STR = 83,         /* builtin_control_vec_generated.go:209 (cond is Int; value args String)            */
    TSQ_OP_IN_STR = 84          /* builtin_other_vec_generated.go:97; arg = number of list items                    */
};
/* tsq_expr_op.flags */
#define TSQ_F_LHS_UNSIGNED 1u
#define TSQ_F_RHS_UNSIGNED 2u
#define TSQ_F_FORCE_SIGNED 4u /* SQLMode NO_UNSIGNED_SUBTRACTION (builtin_arithmetic_vec.go:119) */

typedef struct tsq_expr_op {
    uint8_t  opcode;
    uint8_t  flags;
    uint16_t arg;      /* column index / const index / IN item count */
    uint32_t aux;      /* IN_INT: bitmask of unsigned list items (bit j-1 for item j) */
} tsq_expr_op;

#define TSQ_EXPR_MAX_OPS 64
#define TSQ_EXPR_MAX_STACK 12
#define TSQ_EXPR_MAX_CONSTS 32
#define TSQ_EXPR_STR_POOL 256

/* One expression tree in postfix form.  result_type: TSQ_I64 (Int, also used for U64), TSQ_F64, or TSQ_BYTES for a STRING-valued
 * root — builtinIfStringSig / builtinIfNullStringSig.vecEvalString (builtin_control_vec_generated.go:209, :81), a string column
 * (Column.VecEvalString, column.go:111) or constant (constant.go:86) — which tsq_expr_eval_str evaluates into a var-len column;
 * tsq_expr_eval takes Int and Real roots only; tsq_filter_eval and the join's conditions / filters (ABI 8) also take a string-valued
 * conjunct, whose truth is types.StrToInt(value) != 0 (expression.go:281-326 toBool, ETString arm) under the flags of str_ctx. */
typedef struct tsq_expr_prog {
    int32_t     n_ops;
    int32_t     n_consts;
    int32_t     result_type;
    int32_t     result_unsigned; /* UNSIGNED flag of the result FieldType (informational) */
    tsq_expr_op ops[TSQ_EXPR_MAX_OPS];
    int64_t     consts[TSQ_EXPR_MAX_CONSTS]; /* int64, the bit pattern of a double, or (offset << 32 | length) of a string constant */
    int32_t     n_str_bytes;                 /* bytes used in str_pool */
    int32_t     str_ctx;                     /* ABI 8: TSQ_STRCTX_* bits, the statement's string-to-int flags (0 = a SELECT) */
    uint8_t     str_pool[TSQ_EXPR_STR_POOL]; /* the bytes of the string constants */
} tsq_expr_prog;

/* tsq_expr_prog.str_ctx: the StatementContext flags types.StrToInt reads (executor/executor.go:609-680 ResetContextOfStmt sets them).
 * 0 is a SELECT: CastStrToIntStrict, TruncateAsWarning.  Any other bit -> TSQ_ERR_INVALID at compile. */
#define TSQ_STRCTX_NOT_STRICT       1  /* !CastStrToIntStrict: the float prefix path (types/convert.go:252-257, :318-403)           */
#define TSQ_STRCTX_TRUNCATE_ERROR   2  /* !TruncateAsWarning: a truncation is an error (types/datum.go:948-957)                      */
#define TSQ_STRCTX_IGNORE_TRUNCATE  4  /* IgnoreTruncate: a truncation is neither a warning nor an error                            */
#define TSQ_STRCTX_EMPTY_NOT_ZERO   8  /* neither InSelectStmt nor InDeleteStmt: "" is not read as "0" by the float prefix (:431-433) */
#define TSQ_STRCTX_ALL             15

typedef struct tsq_expr tsq_expr;

/* Compile = validate + upload.  n_progs > 1 is a CNF list (expression.CNFExprs) for filters. */
tsq_status tsq_expr_compile(tsq_ctx* ctx, const tsq_expr_prog* progs, int32_t n_progs, tsq_expr** out);
/* Projection form (evaluator.go:121 / expression.go:329 VecEval): evaluates progs[0] over
 * nrows logical rows; `sel` (optional, int32[nrows]) is chunk.Chunk.sel (chunk.go:319-331).
 * out->data/out->null_bitmap must be sized for nrows; out->type F64 or I64.
 * div_by_zero_warnings (optional) receives the number of x/0 rows (errors.go:65-77). */
tsq_status tsq_expr_eval(tsq_expr* e, const tsq_col* in_cols, int32_t n_cols, int64_t nrows,
                         const int32_t* sel, tsq_col* out, int64_t* div_by_zero_warnings);
/* String-valued root (prog.result_type TSQ_BYTES): the result is a var-len column — ProjectionExec's evaluatorSuite on an ETString
 * expression (executor/projection.go:160, expression/evaluator.go:54-133 -> VecEvalString, expression.go:329-341).  Replaces
 * builtinIfStringSig / builtinIfNullStringSig.vecEvalString (expression/builtin_control_vec_generated.go:209, :81: per row
 * AppendNull or AppendString of the chosen argument), Column.VecEvalString (column.go:111: CopyReconstruct through sel) and
 * Constant.VecEvalString (constant.go:86: the value n times).  out->offsets holds nrows + 1 entries, out->data cap_bytes bytes,
 * out->null_bitmap (nrows + 7) / 8 bytes; same placement (host / TSQ_COL_DEVICE) as the inputs.  *bytes_out = the data bytes of
 * the result; cap_bytes < that (0: only ask) -> nothing but *bytes_out is written and the call returns TSQ_ERR_INVALID.  A NULL row
 * has no bytes (offsets repeat) and a clear bitmap bit, as AppendNull leaves it (util/chunk/column.go:150-158). */
tsq_status tsq_expr_eval_str(tsq_expr* e, const tsq_col* in_cols, int32_t n_cols, int64_t nrows, const int32_t* sel, tsq_col* out,
                             int64_t cap_bytes, int64_t* bytes_out, int64_t* div_by_zero_warnings);
/* Filter form (chunk_executor.go:196 VectorizedFilter / expression.go:205 VecEvalBool):
 * selected_out[i] (one byte per row, Go []bool) = row passes every conjunct, non-NULL.
 * isnull_out (optional) mirrors VecEvalBool's `nulls` for Int-typed conjuncts.
 * ABI 8, string-valued conjuncts (result_type TSQ_BYTES): a NULL drops the row (as for Real), any other value keeps it iff
 * types.StrToInt(value) != 0 under progs[e].str_ctx.  The rows are the nrows logical rows of this call (the ones the
 * division-by-zero count covers), in order: a conjunct fails iff the LAST non-NULL row that reached it raised a conversion
 * error (toBool keeps only that row's error) — TSQ_ERR_OVERFLOW_BIGINT or TSQ_ERR_TRUNCATED_WRONG_VALUE; an evaluation error
 * of the same or an earlier conjunct comes first.  The warnings StrToInt appends are counted: tsq_expr_str_warnings. */
tsq_status tsq_filter_eval(tsq_expr* e, const tsq_col* in_cols, int32_t n_cols, int64_t nrows,
                           const int32_t* sel, uint8_t* selected_out, uint8_t* isnull_out,
                           int64_t* div_by_zero_warnings);
/* Kernel selection.  TSQ_JIT_AUTO (default): once a handle has seen >= 256 Ki rows its programs are compiled into
 * specialised kernels with hiprtc (same source as the interpreter, programs as compile-time constants: the node loop
 * unrolls and every opcode switch folds) — on a helper thread: no call waits for the compile (~250 ms per distinct tree and
 * context, cached), the generic interpreter kernels serve the handle until the code object is there, and they keep serving
 * smaller inputs and any hiprtc failure (tsq_last_error(e) after tsq_expr_jit_launches tells why).  TSQ_JIT_FORCE compiles
 * inside the first call.  Results are identical by construction. */
#define TSQ_JIT_AUTO  (-1)
#define TSQ_JIT_OFF     0
#define TSQ_JIT_FORCE   1
tsq_status tsq_expr_set_jit(tsq_expr* e, int32_t mode);
int64_t    tsq_expr_jit_launches(tsq_expr* e);   /* number of launches served by specialised kernels so far */
double     tsq_expr_jit_compile_ms(tsq_expr* e); /* ABI 7: what hiprtc + the module load of this handle's programs took (0: not compiled yet, or found
                                                  * in the context's cache of program sets; a tree is compiled once per context) */
/* ABI 8: the warnings the string conjuncts of the most recent tsq_filter_eval of this handle raised, one per row and kind
 * (types.StrToInt: ErrTruncatedWrongVal, and ErrOverflow "BIGINT" of an exponent beyond 21 digits, types/convert.go:362-369); the
 * shim appends that many of each to the statement context (AppendWarning stops at 65535).  Conjuncts after a failing one count none. */
tsq_status tsq_expr_str_warnings(tsq_expr* e, int64_t* truncated, int64_t* overflow);
void       tsq_expr_destroy(tsq_expr* e);

/* ---------------------------------------------------------------- hash join
 * Replaces HashJoinExec (executor/join.go:31-60): fetchAndBuildHashTable (:148-158, STUB in the
 * reference), hashRowContainer.PutChunk/GetMatchedRows (hash_table.go:110-169), join2Chunk
 * (join.go:325-362) and the joiners (joiner.go:220-410). */
enum { TSQ_JOIN_INNER = 0, TSQ_JOIN_LEFT_OUTER = 1, TSQ_JOIN_RIGHT_OUTER = 2 }; /* joiner.go:105-116 */

#define TSQ_MAX_KEYS 4
#define TSQ_MAX_COLS 16

typedef struct tsq_join_cfg {
    int32_t join_type;
    /* which child is the build (inner/hashed) side: 1 = right child (probe = left).
     * Output column order is ALWAYS left-child cols || right-child cols (joiner.go:145-150). */
    int32_t build_is_right;
    int32_t n_keys;
    int32_t build_key_idx[TSQ_MAX_KEYS];
    int32_t probe_key_idx[TSQ_MAX_KEYS];
    int32_t n_build_cols;
    int32_t n_probe_cols;
    int32_t build_types[TSQ_MAX_COLS];  /* TSQ_I64.. per build-side column */
    int32_t probe_types[TSQ_MAX_COLS];
    int64_t est_build_rows;             /* innerSideEstCount (hash_table.go:84-96); 0 = unknown */
    int32_t max_chunk_size;             /* tidb_max_chunk_size (tidb_vars.go:242), default 1024 */
    int32_t concurrency;                /* tidb_hash_join_concurrency; unused on the GPU (kept for parity of cfg) */
    int64_t probe_batch_rows;           /* rows staged per device batch; 0 = default (4Mi) */
    /* OtherConditions evaluated on the joined row (lhs||rhs) (joiner.go:155-167); may be NULL */
    const tsq_expr_prog* other_conds;
    int32_t n_other_conds;
    /* outerSideFilter over the probe-side schema (join.go:328); may be NULL */
    const tsq_expr_prog* outer_filters;
    int32_t n_outer_filters;
} tsq_join_cfg;

typedef struct tsq_join tsq_join;

tsq_status tsq_join_create(tsq_ctx* ctx, const tsq_join_cfg* cfg, tsq_join** out);
/* Build side: one call per inner-child chunk (hashRowContainer.PutChunk, hash_table.go:146).
 * Rows whose key has a NULL are kept for outer-join output but never inserted (:161-163). */
tsq_status tsq_join_build_push(tsq_join* j, const tsq_col* cols, int32_t n_cols, int64_t nrows);
tsq_status tsq_join_build_finish(tsq_join* j);
/* The build side of a COUNT(*) join SHARDED over the GPUs of a node, without moving a single probe row.
 * COLLECTIVE: every rank of `comm` pushes ITS build rows (tsq_join_build_push) and then calls this instead of
 * tsq_join_build_finish.  The ranks agree on the key range of the whole build side (two 8-byte all-reduces), every rank
 * assembles the packed direct-address images (csrc/tsq_dajoin.h) of its rows over that range, and the images are summed across
 * the ranks with ONE all-reduce (2^b bytes, or 2^b / 8 for a build side without duplicate keys: 128 MiB for 8e8 keys).  Every
 * rank then holds the images of the WHOLE build side: tsq_join_probe_push takes the rank's OWN probe rows, tsq_join_count the
 * rank's joined rows (the plan adds them up, tsq_comm_allreduce_i64) — the probe phase puts nothing on xGMI and scales with the
 * number of GPUs.  Replaces the N join workers probing ONE shared, read-only hashRowContainer (executor/join.go:233-239,
 * hash_table.go:110-134): the images are that container, replicated because HBM is not shared between GPUs.
 * *shared_out = 1: done — the handle is count-only.  *shared_out = 0 (the same on every rank): the build side is not packable
 * (outer join / conditions / several or non-integer key columns, a key range beyond 31 bits or too sparse, more than 255 build
 * rows per key, duplicate keys in a range beyond 28 bits) — nothing was built, the handle still holds the pushed rows
 * (tsq_join_build_finish makes it a LOCAL join); a distributed plan destroys it and redistributes both sides by rank(key)
 * (tsq_redistribute), as tinysql_amd/parallel.py does. */
typedef struct tsq_comm tsq_comm;
tsq_status tsq_join_build_finish_shared(tsq_join* j, tsq_comm* comm, int32_t* shared_out);
/* Probe side: one call per outer-child chunk (join2Chunk, join.go:325). `selected` (optional,
 * one byte per row) is an externally evaluated outer-side filter; rows with selected==0 or a
 * NULL key go to onMissMatch (join.go:344-345). */
tsq_status tsq_join_probe_push(tsq_join* j, const tsq_col* cols, int32_t n_cols, int64_t nrows,
                               const uint8_t* selected);
tsq_status tsq_join_probe_finish(tsq_join* j);
/* HashJoinExec.Next (join.go:125-146): fills up to cap_rows joined rows into out_cols
 * (n_cols == n_probe_cols + n_build_cols, left||right order, host or device buffers).
 * *nrows_out == 0 && *eos == 0  -> needs more probe input;  *eos == 1 -> end of stream. */
tsq_status tsq_join_pull(tsq_join* j, tsq_col* out_cols, int32_t n_cols, int64_t cap_rows,
                         int64_t* nrows_out, int32_t* eos);
/* Var-len (TSQ_BYTES) columns travel through the join as payload (util/chunk/column.go:28-34: offsets + data; Chunk.AppendRow,
 * chunk.go:334-356); join KEYS are fixed width.  A pull fills out_cols[c].offsets (cap_rows + 1 entries) and .data of such a
 * column; tsq_join_peek tells, for the next pull of up to cap_rows rows, how many rows it will deliver and how many data bytes
 * each var-len output column needs (bytes_out[c]; 0 for fixed-width columns), so the caller can size .data first. */
tsq_status tsq_join_peek(tsq_join* j, int64_t cap_rows, int64_t* nrows_out, int64_t* bytes_out, int32_t n_cols);
/* COUNT(*) fast path (config C1: SELECT count(*) FROM t1 JOIN t2 ON t1.k=t2.k): number of
 * joined rows produced so far by probe_push'd input, without materialising them.
 * Valid instead of (not mixed with) tsq_join_pull. */
/* Inline projection (column pruning, planner/core/rule_column_pruning.go): used[c] = 0 tells the operator that the parent never
 * reads output column c (left child's columns, then right child's): routes that gather their output through (probe row,
 * build row) pairs do not materialise it, tsq_join_pull does not touch its buffer (TSQ_COL_BORROW: data = NULL).  A route that
 * writes whole rows anyway may still fill it.  used = NULL: every column is used (default).  Before the first probe row. */
tsq_status tsq_join_set_used_columns(tsq_join* j, const uint8_t* used, int32_t n_cols);
tsq_status tsq_join_set_count_only(tsq_join* j, int32_t on);
tsq_status tsq_join_count(tsq_join* j, int64_t* rows_out);
/* Order-independent checksum of the joined rows seen so far in count-only mode:
 * sum and xor over joined rows of rowhash(all output columns) — parity at full size. */
tsq_status tsq_join_checksum(tsq_join* j, uint64_t* sum_out, uint64_t* xor_out);
tsq_status tsq_join_set_checksum(tsq_join* j, int32_t on);
/* Probe strategy of the COUNT(*) fast path.  TSQ_RADIX_AUTO (default): probe batches that are large
 * enough are radix partitioned by the top bits of the key hash (LDS-staged, write combined) and probed
 * partition by partition so that every XCD works inside a table slice that fits its L2; small batches
 * and small tables take the direct probe.  The same switch, when set before tsq_join_build_finish, selects
 * the BUILD strategy: AUTO assembles the table slice by slice in LDS (two radix passes over key words +
 * row ids, then one LDS image per slice) for single-key builds of >= 4 Mi rows and inserts row by row
 * (64-bit CAS) otherwise.  OFF / FORCE exist for tests and measurements; the joined rows are identical
 * either way.  Replaces the worker dispatch of executor/join.go:160-231 and PutChunk (hash_table.go:146-169). */
#define TSQ_RADIX_AUTO  (-1)
#define TSQ_RADIX_OFF     0
#define TSQ_RADIX_FORCE   1
tsq_status tsq_join_set_radix(tsq_join* j, int32_t mode);
/* Key packing of the radix probe (round 3; csrc/tsq_dajoin.h).  The build side is complete before the first probe row, so the
 * range [kmin, kmax] of its key column is known.  TSQ_RADIX_AUTO (default): when the key is ONE integer column on both sides,
 * the range fits 28 bits, holds >= 1 build row per 32 values and no key has more than 255 build rows, a COUNT(*) probe batch
 * travels as 2-byte entries (bijective mix of key - kmin; partition = its top bits) and meets a direct-address table of one
 * byte per value of the range, one 64 KB image per partition in LDS — equality of entries IS equality of keys
 * (util/codec/codec.go:363-382), a probe key outside the range joins nothing.  A build side WITHOUT duplicate keys may span up to
 * 31 bits for a COUNT(*) probe: one BIT per value (4-byte entries).  Materialising probes of inner / outer joins (8-byte columns,
 * OtherConditions of inner joins — and of outer joins over a build side without duplicate keys — included) take the same entries with the probe columns travelling next to them (<= 27 bits).
 * Several integer key columns (<= 4, fields adding up to <= 28 bits) are composed into one key column first and take the same routes.
 * OFF keeps 64-bit table words; FORCE drops the
 * size and density conditions (tests).  Must be chosen before the first probe batch.  The joined rows are identical either way.
 * Replaces join2Chunk + GetMatchedRows (executor/join.go:343-360, hash_table.go:110-134) for that shape. */
tsq_status tsq_join_set_key_packing(tsq_join* j, int32_t mode);
/* Ordered output: joined rows come out in probe-row order (the order of the probe pushes and of the rows inside them), the
 * matches of one probe row in build-row order (the order of the build pushes).  With both children sorted on the join keys
 * and the OUTER child as probe side this is exactly MergeJoinExec's output order (executor/merge_join.go:257-310: outer
 * rows in order, each with its inner group in order, NULL-key inner rows skipped :148-156, unmatched outer rows padded for
 * outer joins) — the GPU operator does not need the inputs to be sorted to produce it.  Pulls then also preserve it. */
tsq_status tsq_join_set_ordered(tsq_join* j, int32_t on);
tsq_status tsq_join_cancel(tsq_join* j);
void       tsq_join_destroy(tsq_join* j);

/* ---------------------------------------------------------------- hash aggregation
 * Replaces HashAggExec (executor/aggregate.go:134-155): partial workers' updatePartialResult
 * (:332-350), getGroupKey (:359-394), shuffleIntermData (:354, STUB), consumeIntermData (:424,
 * STUB), getFinalResult (:429-457) and the executor/aggfuncs package. */
enum {
    TSQ_AGG_COUNT = 0,      /* aggfuncs/func_count.go    */
    TSQ_AGG_SUM = 1,        /* aggfuncs/func_sum.go      */
    TSQ_AGG_AVG = 2,        /* aggfuncs/func_avg.go      */
    TSQ_AGG_MAX = 3,        /* aggfuncs/func_max_min.go  */
    TSQ_AGG_MIN = 4,
    TSQ_AGG_FIRSTROW = 5    /* aggfuncs/func_first_row.go */
};
/* expression/aggregation/aggregation.go:82-97 */
enum { TSQ_MODE_COMPLETE = 0, TSQ_MODE_FINAL = 1, TSQ_MODE_PARTIAL1 = 2, TSQ_MODE_PARTIAL2 = 3 };

#define TSQ_MAX_AGGS 16
#define TSQ_MAX_GROUP_KEYS 4

typedef struct tsq_agg_func {
    int32_t func;       /* TSQ_AGG_*                                                          */
    int32_t mode;       /* TSQ_MODE_*; COMPLETE/PARTIAL1 read raw args, FINAL/PARTIAL2 merge   */
    int32_t arg_col;    /* input column; -1 = constant non-NULL arg (COUNT(*) == count(1),
                           parser/parser.y:3258-3262)                                         */
    int32_t arg_col2;   /* AVG in FINAL/PARTIAL2 mode: arg_col = count column, arg_col2 = sum
                           column (func_avg.go:86-113, descriptor.go:70-81)                    */
    int32_t arg_type;   /* TSQ_I64/U64/F32/F64 of the value argument; TSQ_BYTES for COUNT / MAX / MIN /
                           FIRST_ROW of a string (func_max_min.go:312-378, func_first_row.go:193-230)  */
    int32_t reserved;
} tsq_agg_func;

typedef struct tsq_agg_cfg {
    int32_t n_group_keys;
    int32_t group_key_col[TSQ_MAX_GROUP_KEYS];  /* bare input columns (group-by expressions are
                                                   pre-evaluated with tsq_expr_eval)           */
    int32_t group_key_type[TSQ_MAX_GROUP_KEYS];
    int32_t n_aggs;
    tsq_agg_func aggs[TSQ_MAX_AGGS];
    int32_t n_input_cols;
    int32_t input_types[TSQ_MAX_COLS];
    int64_t est_groups;       /* 0 = unknown (table grows by rehash) */
    int32_t max_chunk_size;
    int32_t reserved;
} tsq_agg_cfg;

typedef struct tsq_agg tsq_agg;

tsq_status tsq_agg_create(tsq_ctx* ctx, const tsq_agg_cfg* cfg, tsq_agg** out);
/* One call per child chunk (HashAggPartialWorker.updatePartialResult, aggregate.go:332). */
tsq_status tsq_agg_push(tsq_agg* a, const tsq_col* cols, int32_t n_cols, int64_t nrows);
/* End of child input: finalise groups (consumeIntermData + getFinalResult, aggregate.go:424-457).
 * Returns TSQ_ERR_OVERFLOW_BIGINT if an int64 SUM/AVG left the BIGINT range (func_sum.go:133). */
tsq_status tsq_agg_finish(tsq_agg* a);
/* Update strategy.  TSQ_AGGFAST_AUTO (default): large batches of a single-key aggregate whose functions
 * fit (COUNT/SUM/AVG/MIN/MAX over <= 2 argument columns, firstrow(group key)) are pre-aggregated in LDS
 * — directly when few groups are expected, after a radix partition by group-key hash otherwise — and
 * only the partial groups are merged into the table in HBM (the reference's partial -> shuffle -> final
 * shape, executor/aggregate.go:96-133).  OFF / FORCE exist for tests and measurements; results are the
 * same up to the documented floating-point reordering of SUM/AVG(double). */
#define TSQ_AGGFAST_AUTO  (-1)
#define TSQ_AGGFAST_OFF     0
#define TSQ_AGGFAST_FORCE   1
tsq_status tsq_agg_set_fast(tsq_agg* a, int32_t mode);
/* StreamAggExec (BASELINE.json north star; the reference has only the plan name, planner/core/cbo_test.go:200-212 "StreamAgg"): on != 0
 * before the first row tells the operator that its child delivers rows ORDERED by the group-by items — equal keys are adjacent (NULL
 * equals NULL, +0.0 equals -0.0: the group key of util/codec/codec.go:713-746).  A group is closed by the first row with another
 * key; tsq_agg_pull then returns the groups IN INPUT ORDER, and FIRST_ROW is the first row of its group.  Aggregate functions,
 * modes, NULL / overflow rules, the empty-input default row and the output schema are HashAggExec's (executor/aggregate.go:307-350,
 * 559-588).  No hash table is probed: a row's group = the groups closed so far + the group heads up to the row (csrc/tsq_streamagg.h);
 * a key that comes back after another key opens a NEW group (the child's order is the caller's contract, as in the planner's
 * property enforcement).  Sort an unordered child with tsq_sort_* first (tinysql_amd/executor.py StreamAggExec does). */
tsq_status tsq_agg_set_stream(tsq_agg* a, int32_t on);
/* After tsq_agg_finish: the number of result rows.  Before: the groups the operator's table holds so far — a LOWER bound (the packed
 * route keeps the partial state of a one-key GROUP BY outside the table until finish, tsq_stats.dense_flushes). */
tsq_status tsq_agg_num_groups(tsq_agg* a, int64_t* out);
/* HashAggExec.Next (aggregate.go:559-588): output schema = one column per agg func, in cfg
 * order.  COMPLETE/FINAL emit final values; PARTIAL1/PARTIAL2 emit partial columns (AVG emits
 * two: count then sum).  Group order is unspecified (Go map order in the reference). */
tsq_status tsq_agg_pull(tsq_agg* a, tsq_col* out_cols, int32_t n_cols, int64_t cap_rows,
                        int64_t* nrows_out, int32_t* eos);
/* Strings in the aggregate: a group key may be TSQ_BYTES (getGroupKey: compactBytesFlag + bytes, util/codec/codec.go:738-744;
 * NULL is its own group) and FIRST_ROW / MAX / MIN (binary collation, types.CompareString) / COUNT take a TSQ_BYTES argument;
 * SUM / AVG of a string answer TSQ_ERR_UNSUPPORTED (the planner casts to double first).  The operator keeps the bytes of the
 * var-len input columns it was pushed until it is destroyed.  A pull fills out_cols[c].offsets (cap_rows + 1 entries) and .data
 * of a var-len output column; tsq_agg_peek (after tsq_agg_finish) tells how many rows the next pull of up to cap_rows rows
 * delivers and how many data bytes each var-len output column needs (bytes_out[c]; 0 for fixed-width columns). */
tsq_status tsq_agg_peek(tsq_agg* a, int64_t cap_rows, int64_t* nrows_out, int64_t* bytes_out, int32_t n_cols);
tsq_status tsq_agg_cancel(tsq_agg* a);
void       tsq_agg_destroy(tsq_agg* a);

/* ---------------------------------------------------------------- group ids over 1..16 key columns
 * A dictionary of group keys: rows of 1..TSQ_GROUPID_MAX_KEYS key columns -> dense 32-bit group ids, and the distinct key rows.  Two rows
 * get the same id iff their group keys are equal as getGroupKey / codec.HashGroupKey define it (executor/aggregate.go:359-394,
 * util/codec/codec.go:713-746), column by column: NULL is a value of its own (not 0, not ""); integers compare by their 8 bytes; F32 is
 * widened to double; doubles compare by the memcomparable image (-0.0 and +0.0 share a group, NaNs group by their bits); strings by
 * length and bytes.  Equality is decided on the cells, never on a hash.  Ids are handed out in order of FIRST OCCURRENCE — row order
 * within a call, call order across calls — so ids and dictionary are deterministic; an id once given never changes.  Limits: fewer
 * than 2^31 rows per call, a table of at most 2^32 slots that is at most half full (2^31 groups); beyond: TSQ_ERR_UNSUPPORTED. */
#define TSQ_GROUPID_MAX_KEYS 16
typedef struct tsq_groupid tsq_groupid;
/* n_keys < 1: TSQ_ERR_INVALID; n_keys > TSQ_GROUPID_MAX_KEYS: TSQ_ERR_UNSUPPORTED.  est_groups = 0: unknown (the table grows) */
tsq_status tsq_groupid_create(tsq_ctx* ctx, const int32_t* key_types, int32_t n_keys, int64_t est_groups, tsq_groupid** out);
/* key_cols: TSQ_COL_DEVICE columns of the handle's types (any of TSQ_I64 / U64 / F32 / F64 / BYTES, null bitmaps allowed);
 * ids_out: device memory, nrows uint64 words (row r: the id of its group) */
tsq_status tsq_groupid_assign(tsq_groupid* g, const tsq_col* key_cols, int32_t n_keys, int64_t nrows, uint64_t* ids_out);
tsq_status tsq_groupid_count(tsq_groupid* g, int64_t* n_groups);
/* the dictionary: one device column per key, row g = the key cells of the FIRST row that brought group g; BORROWED (TSQ_COL_BORROW's
 * rule): the pointers lead into the handle's buffers and stay valid until the next assign / destroy */
tsq_status tsq_groupid_keys(tsq_groupid* g, tsq_col* out_cols, int32_t n_keys, int64_t* n_groups);
/* rows assigned so far; rows that met a slot with their tag but another key (the cell comparison sent them on); table growths; GPU time */
tsq_status tsq_groupid_stats(tsq_groupid* g, int64_t* rows, int64_t* collision_rows, int32_t* rehashes, double* kernel_ms);
tsq_status tsq_groupid_cancel(tsq_groupid* g);  /* every later call on the handle answers TSQ_ERR_CANCELLED */
void       tsq_groupid_destroy(tsq_groupid* g);

/* The aggregate over 1..TSQ_GROUPID_MAX_KEYS group keys.  cfg->n_group_keys must be 0; key_cols / key_types: the bare input columns
 * to group by.  n_keys <= TSQ_MAX_GROUP_KEYS: exactly tsq_agg_create with these keys in cfg (the same routes).  More: the keys go
 * through a tsq_groupid to a child aggregate GROUP BY id (one TSQ_U64 key, the same functions and modes, the columns the functions
 * read + the id as its input: more than TSQ_MAX_COLS of them answer TSQ_ERR_UNSUPPORTED here).  Every tsq_agg_* entry point works on
 * the handle; tsq_agg_set_stream answers TSQ_ERR_UNSUPPORTED for more than TSQ_MAX_GROUP_KEYS keys; tsq_stats.build_partitioned
 * reads 5.  SELECT DISTINCT c1..cN is this with one FIRST_ROW per column (planner/core/logical_plan_builder.go:84-127). */
tsq_status tsq_agg_create_keys(tsq_ctx* ctx, const tsq_agg_cfg* cfg, const int32_t* key_cols, const int32_t* key_types, int32_t n_keys,
                               tsq_agg** out);

/* ---------------------------------------------------------------- device-chunk hand-off between GPU operators
 * Dense copy of the selected rows of a DEVICE-resident chunk (selected[]: one byte per row, device memory, e.g. the
 * output of tsq_filter_eval on device columns).  Replaces SelectionExec's copy of selected rows (executor/executor.go:
 * 393-438) / Column.CopyReconstruct (util/chunk/column.go:504-552) when parent and child are both GPU operators, so a
 * filtered chunk reaches the join / aggregate without leaving HBM.  out_cols must be sized for nrows rows; the selected
 * rows keep their input order (every wave owns a contiguous run of rows and the waves' output ranges follow each
 * other), as SelectionExec and CopyReconstruct guarantee. */
tsq_status tsq_chunk_compact(tsq_ctx* ctx, const tsq_col* cols, int32_t n_cols, int64_t nrows, const uint8_t* selected,
                             tsq_col* out_cols, int64_t* nrows_out);

/* Device-side append (Chunk.Append, util/chunk/chunk.go:302-332, between two DEVICE chunks): rows [0, n) of src_cols go behind the
 * dst_rows rows dst_cols hold.  Same column types on both sides; dst_cols[c].length = the rows the destination's buffers have room for
 * (at least dst_rows + n, else TSQ_ERR_INVALID); a destination column that may receive a NULL needs a null_bitmap (a source without one
 * appends set bits); a string column: dst offsets hold dst_rows + 1 valid entries (none needed when dst_rows = 0), dst_cap_bytes[c] = the
 * bytes its data buffer holds (TSQ_ERR_INVALID "no room" when the cells do not fit; nothing of that column is written), and the source's
 * offsets may start anywhere.  dst_cap_bytes may be NULL without string columns. */
tsq_status tsq_chunk_append(tsq_ctx* ctx, const tsq_col* dst_cols, int64_t dst_rows, const int64_t* dst_cap_bytes, const tsq_col* src_cols,
                            int32_t n_cols, int64_t n);
/* dst[i] |= src[i] for n device bytes: two flag arrays (one byte per row, e.g. of tsq_rows_equal) into one */
tsq_status tsq_bytes_or(tsq_ctx* ctx, uint8_t* dst, const uint8_t* src, int64_t n);

/* ---------------------------------------------------------------- fused Selection + Projection over device chunks (ABI 10)
 * SELECT e1, .., em FROM t WHERE f1 AND .. AND fk as ONE operator: ProjectionExec over SelectionExec, whose EvaluatorSuite.Run
 * evaluates the whole SELECT list per chunk on the rows the selection kept (expression/evaluator.go:46-63, :121-133,
 * executor/executor.go:393-438).  The filter runs once (exactly tsq_filter_eval: a NULL conjunct drops the row, string-valued
 * conjuncts as in ABI 8, the same errors and StrToInt warnings); then one kernel evaluates ALL output programs for every selected
 * row — each input cell is loaded once per row whatever number of programs read it — and writes only the outputs, dense and in
 * input order (output row r = the r-th selected input row).  No compacted copy of the input chunk exists.
 *   filters : CNF list, n_filters 0..16 (0 = a pure projection: no flags, no positions pass)
 *   outputs : 1..16 programs, each with an Int, Real or string-valued (TSQ_BYTES) root
 * Result columns: Int root -> 8-byte TSQ_I64 (TSQ_U64 when result_unsigned), Real root -> TSQ_F64 (a bare F32 column is widened),
 * string-valued root -> a var-len column (offsets + bytes; a NULL row has no bytes and a clear bit). */
typedef struct tsq_project tsq_project;
tsq_status tsq_project_create(tsq_ctx* ctx, const tsq_expr_prog* filters, int32_t n_filters,
                              const tsq_expr_prog* outputs, int32_t n_outputs, tsq_project** out);
/* in_cols must be device resident (TSQ_COL_DEVICE; anything else: TSQ_ERR_INVALID).  out_cols (n_out_cols == n_outputs) are
 * BORROWED, with the meaning of TSQ_COL_BORROW: the call sets data, null_bitmap, offsets, length, type, elem_size and flags of
 * every out_cols[j] to device buffers the handle owns, valid until the next run or the destroy of this handle; the caller sizes
 * nothing (it cannot know how many rows survive).  *nrows_out = the selected rows.  A failing filter returns its error and no
 * output is evaluated.  A row the filter dropped raises no error and counts no division by zero; *div_by_zero_warnings = the
 * filters' count + the outputs' count.  When several outputs fail, the status is that of the smallest output index
 * (defaultEvaluator.run returns at the first failing expression, evaluator.go:49-53).  nrows == 0 or no row selected: TSQ_OK,
 * *nrows_out = 0, outputs of length 0. */
tsq_status tsq_project_run(tsq_project* p, const tsq_col* in_cols, int32_t n_cols, int64_t nrows,
                           tsq_col* out_cols, int32_t n_out_cols, int64_t* nrows_out, int64_t* div_by_zero_warnings);
tsq_status tsq_project_set_jit(tsq_project* p, int32_t mode);   /* TSQ_JIT_AUTO / OFF / FORCE, for the filter and the output kernel alike */
/* the warnings of the string conjuncts of the filters in the most recent run (see tsq_expr_str_warnings) */
tsq_status tsq_project_str_warnings(tsq_project* p, int64_t* truncated, int64_t* overflow);
/* eval_launches: launches of the evaluate-and-scatter kernel (exactly one per run with at least one selected row, whatever the number
 * of outputs); jit_launches: those served by the specialised form; eval_kernel_ms: device time of the most recent one */
tsq_status tsq_project_stats(tsq_project* p, int64_t* eval_launches, int64_t* jit_launches, double* eval_kernel_ms);
void       tsq_project_destroy(tsq_project* p);

/* ---------------------------------------------------------------- coprocessor response rows -> columns (SURVEY.md §8 f, rank 2)
 * Replaces selectResult.readRowsData (distsql/select_result.go:139-155) + codec.Decoder.DecodeOne (util/codec/codec.go:
 * 623-690) for fixed-width schemas: `rows_data` is the RowsData byte string of a coprocessor response chunk — rows one
 * after the other, every value = flag byte + varint (8/9) | 8 big-endian bytes (3/4/5) | nothing (0 = NULL); both the
 * EncodeValue and the EncodeKey forms are accepted, like DecodeOne.  Decodes at most cap_rows rows into out_cols (host
 * or TSQ_COL_DEVICE buffers sized for cap_rows rows; data + null_bitmap), *bytes_consumed = length of the decoded
 * prefix (the caller keeps the remainder, select_result.go:153).  data_flags: TSQ_COL_DEVICE when rows_data is in HBM.
 * Errors are the reference's, decided by the FIRST offending value in stream order; *nrows_out then holds the complete
 * rows before it (already in out_cols) and *bytes_consumed is 0: TSQ_ERR_INVALID with tsq_last_error =
 * "invalid encoded key" (a row ends early, codec.go:625) | "insufficient bytes to decode value" (number.go:46,122) |
 * "value larger than 64 bits" (number.go:120) | "invalid encoded key flag" (codec.go:683).
 * col_types may contain TSQ_BYTES (ABI 6): a compact-bytes (flag 2, bytes.go:141-160) or memcomparable (flag 1, bytes.go:35-118) datum
 * becomes a var-len cell — out_cols of such a column need offsets[cap_rows + 1] and a data buffer of n_bytes bytes, as for
 * tsq_rows_decode_chunks, whose errors apply ("datum kind does not match the column type", DecodeBytes' messages).  A bytes datum has
 * no bounded length, so the row boundaries of such a stream come from one sequential walk over flags and lengths on the host (a
 * stream in HBM is copied back for it); the values are decoded on the GPU, 64 rows per piece (csrc/tsq_decode.hip). */
tsq_status tsq_rows_decode(tsq_ctx* ctx, const uint8_t* rows_data, int64_t n_bytes, uint32_t data_flags, int32_t n_cols,
                           const int32_t* col_types, tsq_col* out_cols, int64_t cap_rows, int64_t* nrows_out,
                           int64_t* bytes_consumed);

/* The same for a response whose CHUNKS are known, var-len columns included.  The storage side cuts the rows of a response into
 * tipb.Chunks of 64 rows (cop_handler_dag.go:510-519) — selectResult walks them one after the other (select_result.go:102-155).
 * Chunk k = bytes [chunk_offsets[k], chunk_offsets[k+1]) of rows_data (n_chunks + 1 non-decreasing entries); every chunk holds whole
 * rows.  col_types may contain TSQ_BYTES: a compact-bytes datum (flag 2: varint length + bytes, util/codec/bytes.go:141-160 — what
 * a varchar / blob column arrives as) becomes a var-len cell; such an output column needs offsets[cap_rows + 1] and a data buffer of
 * n_bytes bytes (a cell is a piece of the response).  All rows of all chunks are decoded: if they exceed cap_rows nothing is written
 * and the call returns TSQ_ERR_INVALID with *nrows_out = the rows needed.  Errors as for tsq_rows_decode, decided by the first
 * offending value in stream order (*nrows_out = the complete rows before it, already in out_cols); additionally TSQ_ERR_INVALID
 * "datum kind does not match the column type" (a bytes datum for a number column or the reverse).  A memcomparable bytes datum
 * (flag 1: groups of 8 bytes + a marker, util/codec/bytes.go:35-118 — the EncodeKey form index keys hold) becomes a var-len cell too;
 * its errors are DecodeBytes': "insufficient bytes to decode value" | "invalid marker byte" | "invalid padding byte". */
tsq_status tsq_rows_decode_chunks(tsq_ctx* ctx, const uint8_t* rows_data, int64_t n_bytes, const int64_t* chunk_offsets, int64_t n_chunks,
                                  uint32_t data_flags, int32_t n_cols, const int32_t* col_types, tsq_col* out_cols, int64_t cap_rows,
                                  int64_t* nrows_out);

/* ---------------------------------------------------------------- index scans: the pairs of an index range -> columns (SURVEY.md §8 f, rank 4)
 * Replaces mocktikv's indexScanExec loop (store/mockstore/mocktikv/executor.go:191-320) = tablecodec.DecodeIndexKV
 * (tablecodec/tablecodec.go:376-434) per pair + the DecodeOne of every cut value by the executors above it.  Key k = bytes
 * [key_offsets[k], key_offsets[k+1]) of `keys`:  't' | EncodeInt(tableID) | "_i" | EncodeInt(indexID)  (19 bytes, skipped like
 * CutIndexKeyNew does)  | n_index_cols datums in EncodeKey form (ints flag 3, uints 4, reals 5, strings flag 1 + memcomparable
 * groups, NULL 0; the value forms are accepted too, like DecodeOne)  | [the handle as an int datum — a non-unique index].
 * pk_status (tablecodec.PrimaryKeyStatus): 0 = no handle column; 1 / 2 = out column n_index_cols is the handle (TSQ_I64 / TSQ_U64):
 * taken from the key when bytes remain behind the index columns, otherwise from the pair's value (bytes [value_offsets[k],
 * value_offsets[k+1]) of `values`, 8 bytes big endian: DecodeIndexValueAsHandle, tablecodec.go:456-465).
 * col_types / out_cols: n_index_cols (+ 1) entries; out_cols sized for n_keys rows, a TSQ_BYTES column with offsets[n_keys + 1] and
 * a data buffer of n_bytes bytes.  data_flags: TSQ_COL_DEVICE when keys / key_offsets / values / value_offsets are in HBM.
 * Errors are decided by the first offending pair in key order (*nkeys_out = the pairs before it, already in out_cols):
 * TSQ_ERR_INVALID "invalid encoded key" (a key shorter than its prefix + columns) | the DecodeOne errors of tsq_rows_decode_chunks |
 * "no handle in index key or value". */
tsq_status tsq_indexkeys_decode(tsq_ctx* ctx, const uint8_t* keys, int64_t n_bytes, const int64_t* key_offsets, int64_t n_keys,
                                const uint8_t* values, int64_t n_value_bytes, const int64_t* value_offsets, uint32_t data_flags,
                                int32_t n_index_cols, const int32_t* col_types, int32_t pk_status, tsq_col* out_cols, int64_t* nkeys_out);

/* ---------------------------------------------------------------- the chunk wire format (SURVEY.md §8 a/A "wire Codec", f rank 2)
 * Replaces chunk.Codec (util/chunk/codec.go:28-143) and chunk.Decoder (codec.go:233-353) on device chunks.  A wire chunk is its
 * columns one after the other, each  u32 length | u32 nullCount | [(length + 7) / 8 bitmap bytes, only when nullCount > 0] |
 * [(length + 1) int64 offsets, var-len only] | data  — little endian, no padding (codec.go:50-76).  This is the column-major response
 * format a coprocessor can answer with instead of datum rows (tsq_rows_decode*): decoding it is a copy.
 *
 * tsq_chunk_encode = Codec.Encode (codec.go:42-48): cols (host, or TSQ_COL_DEVICE) -> out (host, or device with out_flags =
 * TSQ_COL_DEVICE).  *bytes_out = the encoded length; cap_bytes = 0 only asks for it; a too small buffer -> TSQ_ERR_INVALID with
 * *bytes_out set.  A column whose bitmap has no zero bit in its first nrows bits travels without it (nullCount = 0).
 *
 * tsq_chunk_decode = Codec.DecodeToChunk (codec.go:88-93) followed by Decoder.Decode (codec.go:257-269, 298-353): rows
 * [first_row, first_row + max_rows) of the wire chunk (cut at its end) are APPENDED to out_cols behind the out_cols[c].length rows
 * they already hold — data copied, var-len offsets rebased onto offsets[length] (an empty destination gets offsets[0] = 0), bitmap
 * bits shifted to the destination's bit position with the bits beyond the last row cleared; a column without a wire bitmap appends
 * set bits.  first_row must be a multiple of 8 (the Decoder consumes its intermediate chunk in multiples of 8 rows, codec.go:259);
 * the buffers of out_cols must hold length + max_rows rows (tsq_chunk_decode_peek tells the data bytes of the var-len columns).
 * out_cols[c].length is updated, *nrows_out = rows appended, *bytes_consumed = the length of the wire chunk (n_cols columns; the
 * caller keeps the remainder, codec.go:93).  first_row = 0, max_rows >= length on empty out_cols is DecodeToChunk / ReuseIntermChk.
 * A HOST buffer is staged into HBM by every call (the whole wire chunk): a Decoder that takes its response window by window uploads it
 * once (tsq_dev_alloc + tsq_copy_h2d) and passes data_flags = TSQ_COL_DEVICE.
 * Errors: TSQ_ERR_INVALID when the buffer ends inside a column, the offsets of a var-len column are damaged, or the columns have
 * different lengths (the reference slices out of range and panics). */
tsq_status tsq_chunk_encode(tsq_ctx* ctx, const tsq_col* cols, int32_t n_cols, int64_t nrows, uint8_t* out, int64_t cap_bytes,
                            uint32_t out_flags, int64_t* bytes_out);
/* rows_total_out: Column.length of the wire chunk; nrows_out: rows the window holds; bytes_out[c]: data bytes of var-len column c in
 * that window (0 for fixed-width columns); any out pointer may be NULL */
tsq_status tsq_chunk_decode_peek(tsq_ctx* ctx, const uint8_t* buf, int64_t n_bytes, uint32_t data_flags, const int32_t* col_types,
                                 int32_t n_cols, int64_t first_row, int64_t max_rows, int64_t* rows_total_out, int64_t* nrows_out,
                                 int64_t* bytes_out, int64_t* bytes_consumed);
tsq_status tsq_chunk_decode(tsq_ctx* ctx, const uint8_t* buf, int64_t n_bytes, uint32_t data_flags, const int32_t* col_types,
                            int32_t n_cols, int64_t first_row, int64_t max_rows, tsq_col* out_cols, int64_t* nrows_out,
                            int64_t* bytes_consumed);

/* ---------------------------------------------------------------- stored rows (rowcodec v2) -> columns (SURVEY.md §8 f, rank 4)
 * Replaces the per-row loop around rowcodec.ChunkDecoder.DecodeToChunk (util/rowcodec/decoder.go:158-238; row.fromBytes /
 * findColID / getData, util/rowcodec/row.go:37-150) — equivalently the storage-side chain BytesDecoder.DecodeToBytes
 * (decoder.go:252-322, mocktikv tableScanExec, store/mockstore/mocktikv/executor.go:124-196) + readRowsData + DecodeOne —
 * a table scan's KV values, each one row in the new row format
 *     [128][flag: bit0 = large][numNotNull u16][numNull u16][colIDs: u8 | u32 each, not-null ids sorted then null ids sorted]
 *     [end offsets of the not-null values: u16 | u32 each][values: ints 1/2/4/8 little-endian bytes, reals 8 bytes memcomparable]
 * become chunk columns.  `values` (n_bytes bytes) holds the rows back to back, row r = bytes [offsets[r], offsets[r+1])
 * (offsets: nrows+1 non-decreasing entries, the last one <= n_bytes), handles[r] = the row's int64 handle from its key (may be NULL when no column is the handle).  data_flags:
 * TSQ_COL_DEVICE when values / offsets / handles are in HBM.  cols[c] describes output column c. */
#define TSQ_RC_HANDLE      1u /* the column is the handle column (col.ID == handleColID, decoder.go:165-168): value = handles[r]   */
#define TSQ_RC_HAS_DEFAULT 2u /* column absent from the row: def_bits instead of NULL (defDatum, decoder.go:186-194)              */
#define TSQ_RC_BIT         4u /* a TypeBit column (type TSQ_BYTES): stored as an unsigned int, the cell is its last byteSize bytes in
                                 big endian (decoder.go:229-231, types.NewBinaryLiteralFromUint); byteSize = (Flen + 7) / 8 in flags bits 8..11 */
#define TSQ_RC_BIT_SIZE(flags) (((flags) >> 8) & 15u)
typedef struct tsq_rowcodec_col {
    int64_t  col_id;    /* ColInfo.ID                                                                                          */
    int32_t  type;      /* TSQ_I64 (signed int types, year), TSQ_U64 (UnsignedFlag), TSQ_F32 (TypeFloat), TSQ_F64 (TypeDouble),
                           TSQ_BYTES (varchar / varstring / string / blobs: chk.AppendBytes of the value, decoder.go:226-228)     */
    uint32_t flags;     /* TSQ_RC_*                                                                                             */
    uint64_t def_bits;  /* default value as it is stored in the column (a float32 default in the low 4 bytes)                  */
    const uint8_t* def_bytes; /* TSQ_BYTES column with TSQ_RC_HAS_DEFAULT: the default string (host memory), def_len bytes       */
    int64_t  def_len;
} tsq_rowcodec_col;
/* out_cols: host or TSQ_COL_DEVICE buffers for nrows rows (data + null_bitmap); a TSQ_BYTES column: offsets[nrows + 1] and a data
 * buffer of n_bytes bytes (a cell is a piece of its row, so the column cannot be larger than `values`) — plus nrows * def_len bytes for
 * a column with a default string (every row may lack the column).  Errors are decided by the FIRST offending
 * row in scan order; *nrows_out then holds the rows before it (already in out_cols): TSQ_ERR_INVALID with tsq_last_error =
 * "invalid codec version" (row.go:54-56) | "insufficient bytes to decode value" (a real shorter than 8 bytes, codec
 * number.go:84-86) | "malformed row" (header / id / offset arrays or a value running past the row, an int value that is not
 * 1, 2, 4 or >= 8 bytes long: the reference panics with an index out of range there). */
tsq_status tsq_rowcodec_decode(tsq_ctx* ctx, const uint8_t* values, int64_t n_bytes, const int64_t* offsets,
                               const int64_t* handles, int64_t nrows, uint32_t data_flags, int32_t n_cols,
                               const tsq_rowcodec_col* cols, tsq_col* out_cols, int64_t* nrows_out);

/* ---------------------------------------------------------------- chunk rows -> coprocessor response bytes (SURVEY.md §8 f, rank 4)
 * The inverse of tsq_rows_decode, for the storage side of a pushed-down plan: replaces the per-datum codec.EncodeValue loop
 * that turns the output rows of the coprocessor's executors into RowsData (store/mockstore/mocktikv/aggregate.go:96-113 for
 * partial aggregates, util/rowcodec/decoder.go:252-322 for scanned rows; cop_handler_dag.go:414-425 concatenates the values of a
 * row).  Row r of the columns `cols` becomes its values' datums back to back — int64 -> varintFlag + zig-zag varint,
 * uint64 -> uvarintFlag + varint, float / double -> floatFlag + 8 memcomparable bytes of the double, a var-len (TSQ_BYTES) cell ->
 * compactBytesFlag + varint(length) + the bytes (codec.go:101-109, bytes.go:141-148), NULL -> NilFlag
 * (util/codec/codec.go:74-99 with comparable = false) — and rows follow each other in `out` (host, or TSQ_COL_DEVICE in
 * out_flags).  col_flags[c] & TSQ_ENC_COMPARABLE selects the EncodeKey form of an integer column (intFlag / uintFlag + 8
 * big-endian bytes): what BytesDecoder.DecodeToBytes emits for the handle column (decoder.go:263-273).  col_flags may be NULL.
 * row_offsets (NULL or nrows + 1 entries, same residency as out): row r = out[row_offsets[r], row_offsets[r + 1]) — the response
 * is cut into tipb.Chunks of 64 rows (cop_handler_dag.go:510-519).  *bytes_out = length of the byte string; when it exceeds
 * cap_bytes nothing is written and the call returns TSQ_ERR_INVALID with *bytes_out = the bytes needed (a caller that cannot bound
 * the size — string columns — asks with cap_bytes = 0 first).  TSQ_ENC_COMPARABLE on a var-len column writes the memcomparable
 * form index keys hold: bytesFlag + groups of 8 bytes, each followed by its marker 0xFF - pad count (codec.go:86-91,
 * bytes.go:35-67).  256 consecutive rows must encode to < 4 GiB. */
#define TSQ_ENC_COMPARABLE 1u
tsq_status tsq_rows_encode(tsq_ctx* ctx, const tsq_col* cols, int32_t n_cols, const uint32_t* col_flags, int64_t nrows,
                           uint8_t* out, int64_t cap_bytes, uint32_t out_flags, int64_t* row_offsets, int64_t* bytes_out);

/* ---------------------------------------------------------------- record keys of a table scan <-> handles (SURVEY.md §8 f, rank 4)
 * Replaces tablecodec.DecodeRowKey (tablecodec/tablecodec.go:235-242; DecodeRecordKey :73-77 hands the table id back as well),
 * called once per scanned KV pair by mocktikv's tableScanExec (store/mockstore/mocktikv/executor.go:124-196) before
 * rd.DecodeToBytes — handles_out[] is the `handles` argument of tsq_rowcodec_decode — and EncodeRowKeyWithHandle (:65-70).
 *     record key = 't' | EncodeInt(tableID) | "_r" | EncodeInt(handle)           RecordRowKeyLen = 19 bytes
 * `keys` holds the keys back to back: key r = bytes [key_offsets[r], key_offsets[r+1]) (n_keys+1 non-decreasing entries), or
 * bytes [19 r, 19 r + 19) when key_offsets is NULL (then n_bytes = 19 * n_keys).  data_flags: TSQ_COL_DEVICE when keys /
 * key_offsets / the outputs are in HBM.  table_ids_out may be NULL.  The FIRST key in scan order that is not a record key
 * (length != 19, no 't' prefix, no "_r" separator) decides: TSQ_ERR_INVALID with tsq_last_error = "invalid key"
 * (errInvalidKey, tablecodec.go:237), *nkeys_out = the keys before it (their handles are out). */
tsq_status tsq_rowkeys_decode(tsq_ctx* ctx, const uint8_t* keys, int64_t n_bytes, const int64_t* key_offsets, int64_t n_keys,
                              uint32_t data_flags, int64_t* handles_out, int64_t* table_ids_out, int64_t* nkeys_out);
/* keys_out: 19 * n_keys bytes, key r = EncodeRowKeyWithHandle(table_id, handles[r]) */
tsq_status tsq_rowkeys_encode(tsq_ctx* ctx, int64_t table_id, const int64_t* handles, int64_t n_keys, uint32_t data_flags,
                              uint8_t* keys_out);

/* ---------------------------------------------------------------- the write path: chunk rows -> stored rows and index entries
 * tsq_rowcodec_encode replaces rowcodec.Encoder.Encode (util/rowcodec/encoder.go:34-194), reached through tablecodec.EncodeRow
 * (tablecodec/tablecodec.go:129) from tables.AddRecord for every row of an INSERT / INSERT .. SELECT / bulk load: the inverse of
 * tsq_rowcodec_decode.  Row r of the columns `cols` (host, or all TSQ_COL_DEVICE), column c under id col_ids[c], becomes
 *     [128][large][numNotNull u16][numNull u16][not-null ids sorted, null ids sorted: u8 | u32][end offsets of the not-null values:
 *     u16 | u32][values]
 * with TSQ_I64 -> 1/2/4/8 little-endian bytes by magnitude (encodeInt), TSQ_U64 -> the same unsigned (encodeUint), TSQ_F32 (widened to
 * double) / TSQ_F64 -> 8 memcomparable bytes (codec.EncodeFloat), TSQ_BYTES -> the bytes as they are, TSQ_BYTES with col_flags[c] =
 * TSQ_RC_BIT (+ byte size) -> the unsigned integer the cell's 1..8 big-endian bytes spell, written like a TSQ_U64 (what
 * tsq_rowcodec_decode reads back as a bit column; any other cell length: TSQ_ERR_INVALID), NULL -> its id among the null ids.
 * col_flags may be NULL.  A row is large (u32 ids and offsets) when a column id exceeds 255 or its value bytes reach 65535.
 * DEPARTURE: at EXACTLY 65535 value bytes the reference turns the row large without widening its offsets (encoder.go:151-157) and the
 * row cannot be decoded; here the row is large with the offsets it means.
 * col_ids: distinct, in [0, 2^32), else TSQ_ERR_INVALID; n_cols: 1..TSQ_MAX_COLS, else TSQ_ERR_INVALID.  A row whose value bytes reach
 * 2^32 answers TSQ_ERR_UNSUPPORTED (the reference wraps silently).  Output, sizing and row_offsets exactly as tsq_rows_encode:
 * *bytes_out is known before a byte is written; cap_bytes too small (0: only ask for the size) -> TSQ_ERR_INVALID with *bytes_out =
 * the bytes needed and nothing written. */
tsq_status tsq_rowcodec_encode(tsq_ctx* ctx, const tsq_col* cols, int32_t n_cols, const int64_t* col_ids, const uint32_t* col_flags,
                               int64_t nrows, uint8_t* out, int64_t cap_bytes, uint32_t out_flags, int64_t* row_offsets,
                               int64_t* bytes_out);

/* tsq_indexkeys_encode replaces index.GenIndexKey (table/tables/index.go:161-189) + the value index.Create stores (:224-244), run per
 * row by the ADD INDEX backfill (ddl/index.go:742-921) and executor/batch_checker.go:127: the inverse of tsq_indexkeys_decode.
 *     key r = 't' | EncodeInt(table_id) | "_i" | EncodeInt(index_id) | EncodeKey(index values of row r) [| the handle as an int datum]
 * EncodeKey = tsq_rows_encode with TSQ_ENC_COMPARABLE on every column.  Row r is DISTINCT when index_flags & TSQ_IDX_UNIQUE and none
 * of its index values is NULL: then the key ends behind the values, distinct_out[r] = 1 and value r = EncodeHandle(handles[r]), 8
 * bytes big endian; otherwise the handle datum follows in the key, distinct_out[r] = 0 and value r = the byte '0'.  Values are
 * written back to back (value r = values_out[value_offsets[r], value_offsets[r + 1]), at most 8 * nrows bytes), the layout
 * tsq_indexkeys_decode takes.  prefix_len[c] >= 0 on a TSQ_BYTES column is TruncateIndexValuesIfNeeded (:127-157): prefix_utf8[c] == 0
 * (binary charset) the first prefix_len bytes of a longer cell; == 1 (utf8 / utf8mb4) the first prefix_len runes of a cell that holds
 * more, runes as Go's utf8.DecodeRune counts them (a byte that does not start a shortest-form, non-surrogate sequence up to U+10FFFF
 * is one rune of width 1).  DEPARTURE: the reference re-encodes a truncated cell through []rune, rewriting each invalid byte of the
 * kept prefix as EF BF BD; a cell that would be truncated and whose kept prefix holds an invalid byte answers TSQ_ERR_UNSUPPORTED
 * (that row keeps the Go path).  A cell that is not truncated is never touched.  Both arrays may be NULL.
 * cols / handles: host, or all in HBM (TSQ_COL_DEVICE on every column); data_flags: TSQ_COL_DEVICE when the five outputs are in HBM.
 * Sizing as tsq_rows_encode on the key bytes (*bytes_out, cap_bytes); n_index_cols: 1..TSQ_MAX_COLS, else TSQ_ERR_INVALID. */
#define TSQ_IDX_UNIQUE 1u
tsq_status tsq_indexkeys_encode(tsq_ctx* ctx, int64_t table_id, int64_t index_id, uint32_t index_flags, const tsq_col* cols,
                                int32_t n_index_cols, const int32_t* prefix_len, const uint8_t* prefix_utf8, const int64_t* handles,
                                int64_t nrows, uint32_t data_flags, uint8_t* keys_out, int64_t cap_bytes, int64_t* key_offsets,
                                uint8_t* values_out, int64_t* value_offsets, uint8_t* distinct_out, int64_t* bytes_out);

/* ---------------------------------------------------------------- INSERT .. SELECT: column casts, NOT NULL checks, auto ids
 * No row of an INSERT .. SELECT reaches tables.AddRecord as the child produced it: insertRowsFromSelect (executor/insert_common.go:
 * 340-381) sends every row through getRow (:386-401) — table.CastValue (table/column.go:142-189) on every cell the statement names,
 * in statement-column order — and fillRow (:455-469) — the default of every column it does not name, then Column.HandleBadNull
 * (table/column.go:290-299), in table-column order.  tsq_cast_run does that for a whole chunk; its output columns are what
 * tsq_rowcodec_encode / tsq_indexkeys_encode take.  tsq_autoid_fill then gives the auto-increment column its values
 * (adjustAutoIncrementDatum, :594-638).
 *
 * cols[c] describes column c of the TABLE, in Table.Cols() order.  The output column of an integer target is a TSQ_I64 column
 * (TSQ_U64 with TSQ_CAST_UNSIGNED), of TypeFloat a TSQ_F32 column, of TypeDouble a TSQ_F64 column.  Per (source, target), bit for bit
 * what CastValue returns:
 *   any source                NULL -> NULL (types/datum.go:492-494)
 *   I64/U64/F32/F64 -> signed ints     toSignedInteger (datum.go:739-757): ConvertIntToInt / ConvertUintToInt / ConvertFloatToInt
 *                             (types/convert.go:93-128) — RoundFloat (types/helper.go:28-34), half away from zero; the value AT the
 *                             upper bound as a float (2^63 for BIGINT) is the bound without an error
 *   I64/U64/F32/F64 -> unsigned ints   convertToUint (datum.go:639-674): ConvertIntToUint (a negative value clips to 0 under
 *                             TSQ_CAST_IN_INSERT, else it wraps and is compared as unsigned) / ConvertUintToUint / ConvertFloatToUint
 *                             (convert.go:131-174) — a float AT the bound of the type answers MaxInt64 without an error and one above
 *                             it MaxInt64 with one, as the reference does for every unsigned type; a negative float without
 *                             TSQ_CAST_IN_INSERT is uint64(int64(val)), 0x8000000000000000 below -2^63 (the amd64 conversion)
 *   I64/U64/F32/F64 -> FLOAT/DOUBLE    convertToFloat + ProduceFloatWithSpecifiedTp (datum.go:516-566): with flen and decimal both
 *                             given TruncateFloat (helper.go:72-94) — Round as f * shift, RoundFloat, / shift, three single IEEE
 *                             operations with shift = math.Pow10(decimal), clipped to +-GetMaxFloat(flen, decimal), NaN -> 0, each
 *                             with ErrOverflow, which sc.HandleOverflow turns into a warning under TSQ_CAST_OVERFLOW_AS_WARNING;
 *                             then TSQ_CAST_UNSIGNED and a negative value -> 0 with an error; TypeFloat narrows to float32
 *   BYTES -> string family    ProduceStrWithSpecifiedTp (datum.go:597-632): flen counts RUNES under TSQ_CAST_CHARSET_UTF8 / _UTF8MB4
 *                             (utf8.RuneCountInString: a byte that starts no valid sequence is one rune) and bytes otherwise; a longer
 *                             value is cut there with ErrDataTooLong; TypeString + TSQ_CAST_CHARSET_BIN (BINARY(n)) is padded with \0 to
 *                             flen.  Then CastValue (table/column.go:159-186): a TypeString without the binary charset loses its
 *                             trailing spaces; unless TSQ_CAST_SKIP_UTF8_CHECK or a charset other than utf8 / utf8mb4, the value is cut at
 *                             its first invalid byte, or at its first 4-byte rune under 3-byte utf8 (a literal EF BF BD is valid), with
 *                             ErrTruncatedWrongValueForField (TSQ_ERR_BAD_UTF8).  Under strict truncation ErrDataTooLong is returned
 *                             before the trim and the walk.  The output is a TSQ_BYTES column
 *   I64/U64 -> string family  strconv.FormatInt / FormatUint, then the same length rules
 *   BYTES -> signed ints      toSignedInteger's string arm (datum.go:751-757): types.StrToInt with the str_ctx flags (TSQ_STRCTX_*), then
 *                             ConvertIntToInt; the clipped value is always stored and StrToInt's error (ErrOverflow "BIGINT", or
 *                             ErrTruncatedWrongVal -> TSQ_ERR_TRUNCATED_WRONG_VALUE) wins over the clip's
 *   BYTES -> unsigned ints    convertToUint's string arm (:654-663): types.StrToUint (convert.go:234-246: StrToInt's prefix, one leading
 *                             '+' stripped, strconv.ParseUint — a '-' in front is its syntax error; either failure is ErrOverflow
 *                             "BIGINT UNSIGNED"); that overflow returns at once unless sc.ShouldIgnoreOverflowError() (TSQ_CAST_IN_INSERT
 *                             and TSQ_CAST_TRUNCATE_AS_WARNING), then ConvertUintToUint, whose error returns at once too, then the parse's
 *                             error goes with the value.  Both early returns carry the reference's ZERO Datum: when HandleTruncate
 *                             swallows the error the cell is NULL (and meets the NOT NULL rule)
 *                             Warnings StrToInt appends itself (a cut prefix under a warning context; an exponent beyond 21 digits)
 *                             count as `truncated` / `overflow`.  The shim passes str_ctx consistent with stmt_flags
 *   src_col = -1              the column's default (def_bits; def_bytes / def_len for a string column, copied at create; NULL with
 *                             TSQ_CAST_DEFAULT_NULL), cast by the host once
 *   then, every column        NULL in a TSQ_CAST_NOT_NULL column: TSQ_ERR_BAD_NULL, or under TSQ_CAST_BAD_NULL_AS_WARNING the zero
 *                             value (GetZeroValue: 0, 0.0, "", flen zero bytes for BINARY(flen)) and a warning.  A TSQ_CAST_AUTO_INCREMENT column is exempt: a NULL
 *                             there (also: not named by the statement) is what tsq_autoid_fill replaces.
 * Error rule: every cast error goes through sc.HandleTruncate (column.go:146-154), overflow included.  TSQ_CAST_IGNORE_TRUNCATE: it
 * vanishes.  TSQ_CAST_TRUNCATE_AS_WARNING: it is counted and the clipped value stands.  Otherwise the run fails with the error of
 * the FIRST failing cell in the reference's order — rows in order; inside a row the casts by statement column (src_col), then the
 * NOT NULL failures by table column — and tsq_cast_error_at names that cell.  After a failed run the output cells of the ROWS IN FRONT
 * of the failing row are what a successful run writes (every cell of every column is computed whatever its neighbours do; a shim
 * uses this to give those rows their ids and find an earlier id error), and so are the cells of the failing row itself
 * when its error is TSQ_ERR_BAD_NULL (a row's casts come before its NOT NULL pass); otherwise that row and the rows behind it are unspecified;
 * tsq_cast_warnings is defined after a run that returned TSQ_OK (the counts of that run).
 * PINNED DEPARTURE: a NaN reaching an integer target (Go's int64(NaN) is implementation defined) fails the run with
 * TSQ_ERR_UNSUPPORTED at that cell, whatever the statement flags.
 * TSQ_ERR_UNSUPPORTED at create — the Go path keeps the statement: a F32 / F64 source into a string target (strconv.FormatFloat's
 * shortest digits), a TSQ_BYTES source into FLOAT / DOUBLE (StrToFloat's correctly rounded parsing), TypeBit targets, an unsigned
 * or floating auto-increment column, more than TSQ_MAX_COLS columns.
 * in_cols / out_cols: host chunks, or all TSQ_COL_DEVICE.  out_cols[c] of a fixed-width column: data for nrows cells and a null_bitmap
 * of (nrows + 7) / 8 bytes.  A string column additionally offsets[nrows + 1] and a data buffer of cap_bytes[c] bytes.  cap_bytes and
 * bytes_out have n_table_cols entries, indexed like cols (entries of fixed-width columns are ignored / set to 0) and are required when
 * the table has a string column.  Sizing as tsq_rowcodec_encode: bytes_out[c] = the data bytes of column c, known before a byte is
 * written; if any exceeds its cap_bytes (0: only ask) NOTHING is written — not the fixed-width columns either — and the call answers
 * TSQ_ERR_INVALID.  Cells of 64 bytes or more are copied by a whole wave.  Output buffers never alias inputs.
 * nrows >= 2^31: TSQ_ERR_UNSUPPORTED. */
typedef struct tsq_cast_col {      /* one column of the TABLE, in table order (Table.Cols()) */
    int32_t  src_col;              /* index into in_cols, or -1: not named by the statement (hasValue = false) */
    int32_t  src_type;             /* TSQ_I64 / U64 / F32 / F64 / BYTES of that input column */
    int32_t  tp;                   /* mysql.Type*: TSQ_TP_TINY .. TSQ_TP_STRING */
    int32_t  flen, decimal;        /* FieldType.Flen / Decimal, -1 = UnspecifiedLength */
    uint32_t flags;                /* TSQ_CAST_UNSIGNED | ... */
    uint64_t def_bits;             /* default of a column with src_col = -1: the 8 bytes of a fixed-width value (TypeFloat: 4) ... */
    const uint8_t* def_bytes; int64_t def_len;   /* ... or the bytes of a string default (already cast by the host, once) */
} tsq_cast_col;
/* mysql.Type* (parser/mysql/type.go) */
#define TSQ_TP_TINY 1
#define TSQ_TP_SHORT 2
#define TSQ_TP_LONG 3
#define TSQ_TP_FLOAT 4
#define TSQ_TP_DOUBLE 5
#define TSQ_TP_LONGLONG 8
#define TSQ_TP_INT24 9
#define TSQ_TP_VARCHAR 15
#define TSQ_TP_BIT 16
#define TSQ_TP_TINY_BLOB 249
#define TSQ_TP_MEDIUM_BLOB 250
#define TSQ_TP_LONG_BLOB 251
#define TSQ_TP_BLOB 252
#define TSQ_TP_VAR_STRING 253
#define TSQ_TP_STRING 254
/* tsq_cast_col.flags */
#define TSQ_CAST_UNSIGNED 1u        /* mysql.UnsignedFlag */
#define TSQ_CAST_NOT_NULL 2u        /* mysql.NotNullFlag / PreventNullInsertFlag */
#define TSQ_CAST_AUTO_INCREMENT 4u  /* mysql.AutoIncrementFlag */
#define TSQ_CAST_CHARSET_BIN 8u     /* charset "binary" */
#define TSQ_CAST_CHARSET_UTF8 16u   /* charset "utf8" (3-byte) */
#define TSQ_CAST_CHARSET_UTF8MB4 32u
#define TSQ_CAST_DEFAULT_NULL 64u   /* the default of a column with src_col = -1 is NULL */
/* statement flags = the StatementContext bits CastValue reads (executor/executor.go ResetContextOfStmt) */
#define TSQ_CAST_IGNORE_TRUNCATE 1u       /* sc.IgnoreTruncate */
#define TSQ_CAST_TRUNCATE_AS_WARNING 2u   /* non-strict mode: clipped value + a warning */
#define TSQ_CAST_OVERFLOW_AS_WARNING 4u   /* HandleOverflow in ProduceFloatWithSpecifiedTp */
#define TSQ_CAST_BAD_NULL_AS_WARNING 8u   /* insert_common.go:350-353 */
#define TSQ_CAST_IN_INSERT 16u            /* ShouldClipToZero / ShouldIgnoreOverflowError (sessionctx/stmtctx/stmtctx.go:359-372) */
#define TSQ_CAST_SKIP_UTF8_CHECK 32u
typedef struct tsq_cast tsq_cast;
/* str_ctx: the TSQ_STRCTX_* flags of types.StrToInt / StrToUint for string -> integer columns (an INSERT: NOT_STRICT | EMPTY_NOT_ZERO, plus
 * TRUNCATE_ERROR or IGNORE_TRUNCATE as the statement flags say) */
tsq_status tsq_cast_create(tsq_ctx* ctx, const tsq_cast_col* cols, int32_t n_table_cols, uint32_t stmt_flags, uint32_t str_ctx, tsq_cast** out);
tsq_status tsq_cast_run(tsq_cast* c, const tsq_col* in_cols, int32_t n_in, int64_t nrows, tsq_col* out_cols /* n_table_cols */,
                        int64_t* cap_bytes /* per var-len output; 0 = ask */, int64_t* bytes_out);
/* position of the error the last run returned (TSQ_ERR_INVALID when it returned none) */
tsq_status tsq_cast_error_at(tsq_cast* c, int64_t* row, int32_t* table_col);
/* overflow: cast overflows kept as warnings (TRUNCATE_AS_WARNING, OVERFLOW_AS_WARNING); data_too_long / bad_utf8: string cells cut to their
 * length / at their first bad byte under TRUNCATE_AS_WARNING; bad_null: NULLs replaced by the zero value; truncated: ErrTruncatedWrongVal of a string -> integer cell kept as a warning */
tsq_status tsq_cast_warnings(tsq_cast* c, int64_t* overflow, int64_t* truncated, int64_t* data_too_long, int64_t* bad_null, int64_t* bad_utf8);
tsq_status tsq_cast_stats(tsq_cast* c, int64_t* rows, int64_t* launches, double* kernel_ms);
tsq_status tsq_cast_cancel(tsq_cast* c);   /* every later call on the handle answers TSQ_ERR_CANCELLED */
void       tsq_cast_destroy(tsq_cast* c);

/* adjustAutoIncrementDatum (executor/insert_common.go:594-638) over the cast output of the auto-increment column (a TSQ_I64 column,
 * host or TSQ_COL_DEVICE), in place, for ONE allocator with increment 1 whose last id is `base` (>= 0, else TSQ_ERR_INVALID).  With s = base,
 * every row in order:
 *   a non-NULL value v != 0 is explicit: the row keeps v, s = max(s, v) (Table.RebaseAutoID), *last_explicit = v (StmtCtx.InsertID);
 *   a NULL, or a 0 without TSQ_AUTOID_NO_AUTO_VALUE_ON_ZERO: s = s + 1, the row becomes s; the first such s is *first_allocated
 *   (lastInsertID); a 0 with the flag stays 0.
 * Every row is NOT NULL afterwards (col->null_bitmap, when given, is rewritten).  *new_base = s: what the shim rebases the real
 * allocator to, once.  *first_allocated / *last_explicit: 0 when there was none.  An allocated id above upper_bound (the column
 * type's, IntergerSignedUpperBound) is the overflow of the re-cast (:633): TSQ_ERR_OUT_OF_RANGE with *error_row = the first such row;
 * s passing INT64_MAX: TSQ_ERR_UNSUPPORTED.  The column is unspecified after either.  Three launches — per-block aggregates, one
 * block scanning them, apply; no workgroup waits for another. */
#define TSQ_AUTOID_NO_AUTO_VALUE_ON_ZERO 1u   /* mysql.ModeNoAutoValueOnZero */
tsq_status tsq_autoid_fill(tsq_ctx* ctx, tsq_col* col, int64_t nrows, int64_t base, uint32_t flags, int64_t upper_bound,
                           int64_t* new_base, int64_t* first_allocated, int64_t* last_explicit, int64_t* error_row);

/* ---------------------------------------------------------------- ORDER BY / TopN (SURVEY.md §8 f, rank 3)
 * Replaces SortExec (executor/sort.go:27-144) and TopNExec (sort.go:146-318): all child rows are pushed, tsq_sort_finish
 * orders them by the ByItems — bare columns (sort.go:107-113), each ascending or descending, compared like
 * chunk.GetCompareFunc's comparators (util/chunk/compare.go:27-103: NULL smaller than every value, unsigned / signed /
 * float32-widened / float64 order) — and tsq_sort_pull hands them out in that order.  limit_count >= 0 makes it a
 * TopN: only rows [limit_offset, limit_offset + limit_count) of the order are returned (sort.go:213-238).  Rows whose
 * keys all compare equal come out in input order (the reference's sort.Slice / heap leave that order unspecified). */
typedef struct tsq_sort_cfg {
    int32_t n_cols;
    int32_t col_types[TSQ_MAX_COLS];
    int32_t n_keys;                       /* ByItems */
    int32_t key_col[TSQ_MAX_KEYS];
    int32_t key_desc[TSQ_MAX_KEYS];       /* ByItems[i].Desc */
    int64_t limit_offset;                 /* PhysicalLimit.Offset (0 for a plain sort) */
    int64_t limit_count;                  /* PhysicalLimit.Count; < 0 = no limit (SortExec) */
    int32_t max_chunk_size;
    int32_t reserved;
} tsq_sort_cfg;
typedef struct tsq_sort tsq_sort;
tsq_status tsq_sort_create(tsq_ctx* ctx, const tsq_sort_cfg* cfg, tsq_sort** out);
tsq_status tsq_sort_push(tsq_sort* s, const tsq_col* cols, int32_t n_cols, int64_t nrows);   /* fetchRowChunks, sort.go:80-97 */
tsq_status tsq_sort_finish(tsq_sort* s);
/* out_cols: the input schema; host or TSQ_COL_DEVICE buffers (data + null_bitmap) for cap_rows rows */
tsq_status tsq_sort_pull(tsq_sort* s, tsq_col* out_cols, int32_t n_cols, int64_t cap_rows, int64_t* nrows_out, int32_t* eos);
/* Var-len (TSQ_BYTES) columns travel through the sort as payload (Chunk.AppendRow of a var-len cell, util/chunk/chunk.go:334-356)
 * and may be ORDER BY items: chunk.GetCompareFunc's cmpString (util/chunk/compare.go:71-77: bytes, then the shorter string first;
 * binary collation, the only one TinySQL has).  A string item costs one radix pass per byte position that differs between rows
 * (plus the length); the TopN radix select takes a string first item by its first eight bytes.  A pull fills out_cols[c].offsets (cap_rows + 1 entries) and .data of a var-len column; tsq_sort_peek (after
 * tsq_sort_finish) tells how many rows the next pull of up to cap_rows rows delivers and how many data bytes each var-len column
 * needs (bytes_out[c]; 0 for fixed-width columns). */
tsq_status tsq_sort_peek(tsq_sort* s, int64_t cap_rows, int64_t* nrows_out, int64_t* bytes_out, int32_t n_cols);
/* rows = rows that went through the radix passes: all of them for a sort; for a TopN whose Offset + Count is small, only the
 * candidates kept by the radix select on the first ORDER BY item (ties at the threshold included) */
tsq_status tsq_sort_stats(tsq_sort* s, int64_t* rows, int32_t* passes, int32_t* passes_skipped, double* sort_kernel_ms);
tsq_status tsq_sort_cancel(tsq_sort* s);
void       tsq_sort_destroy(tsq_sort* s);

/* ---------------------------------------------------------------- IndexLookUp: handle lookup + stored-row gather
 * The storage side of IndexLookUpExecutor's table worker (executor/distsql.go:237-637, the "double read"): an index scan yields
 * handles, the table worker reads those rows of the table.  A TASK is a batch of handles in index-scan order
 * (indexWorker.extractTaskHandles, :510-535).  tsq_lookup_create takes the handles of a table's record keys in scan order — what
 * tsq_rowkeys_decode hands out — device resident (data_flags = TSQ_COL_DEVICE, anything else: TSQ_ERR_INVALID); the library keeps its
 * own copy and the search index it builds over it (TSQ_KNOB_LOOKUP_STRIDE).  n_rows = 0 is legal.  Table order is the order of
 * EncodeInt(handle): SIGNED int64 on the raw 8 bytes of the handle column, also for an unsigned primary key; INT64_MIN and INT64_MAX
 * are ordinary handles.  Handles that are not strictly ascending: TSQ_ERR_INVALID, tsq_last_error(ctx) = "table handles not
 * ascending", no handle is created.
 * tsq_lookup_task: handles (n of them) host, or device with data_flags = TSQ_COL_DEVICE; rows_out / handles_out have the same
 * residency and room for n entries; entries [0, *n_found) are written, nothing else.  rows_out[i] = the table row ordinal of the i-th
 * emitted row, handles_out[i] = its handle (the `handles` argument of tsq_rowcodec_decode).
 *   keep_order = 0: the handles are sorted ascending (builder.go:940) and read as point ranges (distsql/request_builder.go:161-180):
 *                   the rows that exist, in handle order; a missing handle gives nothing, a handle that occurs twice gives its row twice.
 *   keep_order = 1: the rows that exist in TASK order (indexOrder, distsql.go:538-546, 627-634).  DEPARTURE: with a handle occurring
 *                   twice in one task the reference places both rows at the last occurrence's position (indexOrder[h] = i
 *                   overwrites); here each occurrence yields its row at its own position.  An index scan never yields a handle twice.
 * n = 0 and an empty table answer 0 rows; n >= 2^31: TSQ_ERR_UNSUPPORTED.  After tsq_lookup_cancel every call answers TSQ_ERR_CANCELLED.
 * tsq_lookup_stats: tasks and handles taken, rows found, and the device time between the first and the last kernel of the tasks. */
typedef struct tsq_lookup tsq_lookup;
tsq_status tsq_lookup_create(tsq_ctx* ctx, const int64_t* table_handles, int64_t n_rows, uint32_t data_flags, tsq_lookup** out);
tsq_status tsq_lookup_task(tsq_lookup* l, const int64_t* handles, int64_t n, uint32_t data_flags, int32_t keep_order,
                           int64_t* rows_out, int64_t* handles_out, int64_t* n_found);
tsq_status tsq_lookup_stats(tsq_lookup* l, int64_t* tasks, int64_t* handles, int64_t* found, double* kernel_ms);
tsq_status tsq_lookup_cancel(tsq_lookup* l);
void       tsq_lookup_destroy(tsq_lookup* l);
/* The stored rows of a task: all buffers device resident.  Row i of the output = source row rows[i], bytes [offsets[rows[i]],
 * offsets[rows[i] + 1]) of `values` (n_bytes bytes, n_src_rows rows), written back to back into `out`; out_offsets gets n + 1 entries
 * starting at 0 — the values / offsets pair tsq_rowcodec_decode reads.  Sizing as tsq_rows_encode: *bytes_out = the total; when it
 * exceeds cap_bytes nothing is written and the call answers TSQ_ERR_INVALID (a caller asks with cap_bytes = 0 first; out and
 * out_offsets may be NULL then).  A rows[i] outside [0, n_src_rows): TSQ_ERR_INVALID "row index out of range"; an offset pair that
 * decreases or leaves [0, n_bytes]: TSQ_ERR_INVALID too; nothing is read out of bounds and nothing is written in either case.
 * Rows of TSQ_KNOB_GATHER_WAVE_COPY bytes or more are copied by a whole wave. */
tsq_status tsq_rows_gather(tsq_ctx* ctx, const uint8_t* values, int64_t n_bytes, const int64_t* offsets, int64_t n_src_rows,
                           const int64_t* rows, int64_t n, uint8_t* out, int64_t cap_bytes, int64_t* out_offsets, int64_t* bytes_out);

/* ---------------------------------------------------------------- Duplicate keys: INSERT .. SELECT's check and REPLACE .. SELECT
 * The reference checks every row of an INSERT against the store and against the rows the statement wrote before it, one txn.Get per
 * key (table/tables/tables.go:528-581 AddRecord -> CheckHandleExists / index.Create, table/tables/index.go:194-261), and REPLACE
 * removes every row that conflicts with the new one unless it is the very same row (executor/replace.go:53-196,
 * executor/batch_checker.go:66-157).  Here the whole statement is settled at once, with the outcome of the reference's row order.
 *
 * A STREAM is one key that must be unique: the PK handle (kind TSQ_DUP_HANDLE, when PKIsHandle; at most one) or one unique index
 * (TSQ_DUP_INDEX), in the order the reference checks them — the handle first, then WritableIndices order.  1..TSQ_DUP_MAX_STREAMS of
 * them; more: TSQ_ERR_INVALID.  All arrays are DEVICE resident.
 *   HANDLE stream: handles / n = the table's handles in scan order, strictly ascending as signed int64 (tsq_lookup_create's rule and
 *                  its refusal, "table handles not ascending").
 *   INDEX stream : the store's DISTINCT entries of the index (the ones whose value is the 8-byte handle) in key order: keys back to back
 *                  (key_bytes bytes), key_offsets with n + 1 entries starting anywhere inside the keys, handles[e] = the handle entry e
 *                  points to.  Offsets that decrease or leave the keys: TSQ_ERR_INVALID; keys not strictly ascending under memcmp then
 *                  length: TSQ_ERR_INVALID, "index keys not ascending".  flags: TSQ_DUP_FLOAT_KEY when a FLOAT / DOUBLE column is part of
 *                  the index — REPLACE mode refuses such a table with TSQ_ERR_UNSUPPORTED (-0.0 and 0.0 are equal datums with different
 *                  keys, so "equal rows have equal keys" does not hold); INSERT mode takes it.
 *   table_handles / n_table_rows: the table's handles as for a HANDLE stream, for a table WITHOUT one (its _tidb_rowid handles); ignored
 *                  when a HANDLE stream is given.  REPLACE mode names stored rows by their table row ordinal, so every index entry's handle
 *                  must be a row of this table (else tsq_dupcheck_match answers TSQ_ERR_INVALID); INSERT mode does not read it.
 * An empty store (n = 0 everywhere) is legal.  The library COPIES everything it is given at create and at push: the caller's buffers
 * are free again when the call returns.
 *
 * tsq_dupcheck_push appends n statement rows, in statement order: per stream either the rows' handles or their encoded index keys
 * (what tsq_indexkeys_encode writes: keys, n + 1 offsets, and the distinct flags — a key with a NULL cell is not distinct and takes part
 * in nothing; distinct = NULL: all are).  It may be called once per chunk of the select.  2^31 rows, or 2^31 / streams: TSQ_ERR_UNSUPPORTED.
 *
 * tsq_dupcheck_match, INSERT mode: TSQ_OK, or TSQ_ERR_KEY_EXISTS (kv.ErrKeyExists) with *conflict = the smallest failing row, within it
 * the first failing stream, and the entry that was there first: from_store = 1 and dup_handle = the stored entry's handle, or
 * from_store = 0 and dup_row = the FIRST statement row with that key (the one whose entry the failing row met).  A stored entry takes
 * precedence over an in-batch one.  The cand arguments are not read.  REPLACE mode: per statement row r the row EqualDatums has to be asked
 * about, in three device arrays of n entries: cand_row[r] = the latest earlier statement row sharing a distinct key with r in any
 * stream, or -1; when it is -1, cand_ord[r] / cand_handle[r] = table row ordinal and handle of the stored row matched by the FIRST
 * stream that has a match, or -1 / 0.  *n_cand_batch / *n_cand_store count the two kinds.  conflict may be NULL.
 *
 * tsq_dupcheck_resolve (REPLACE mode, after match): equal_flags[r] (device, one byte per row) = EqualDatums(candidate of r, row r);
 * rows without a candidate are not read as equal whatever their flag.  Writes added_out[r] (the row is written: it is not the very same row
 * as its candidate), put_out[r] (added and not removed again by a later added row), handles_out[r] (optional; for a table without
 * a PK handle: rowid_base + the number of added rows up to and including r, 0 for a row that is not added — an unchanged row takes no
 * id), and the stored rows that added rows remove as ascending, distinct (handle, table row ordinal) pairs in removed_handles /
 * removed_ords (room for cap_removed pairs; when more are needed nothing is written, result->n_removed_store says how many, and the
 * call answers TSQ_ERR_INVALID: min(rows * streams, table rows) always suffices).  *result: affected = rows + n_removed_store +
 * n_removed_batch (the reference's affected-rows count), rowid_base = the base after the statement.
 *
 * After tsq_dupcheck_cancel every call answers TSQ_ERR_CANCELLED.  tsq_dupcheck_stats: the rows of the CURRENT statement, the pushes taken
 * since create (tsq_dupcheck_reset clears the rows and the candidate counts, not the pushes and the time), candidates of the two kinds,
 * device time of match + resolve. */
#define TSQ_DUP_MAX_STREAMS 8
#define TSQ_DUP_HANDLE 0
#define TSQ_DUP_INDEX 1
#define TSQ_DUP_INSERT 0
#define TSQ_DUP_REPLACE 1
#define TSQ_DUP_FLOAT_KEY 1u
typedef struct tsq_dup_stream {
    int32_t kind;               /* TSQ_DUP_HANDLE / TSQ_DUP_INDEX */
    uint32_t flags;             /* TSQ_DUP_FLOAT_KEY */
    const int64_t* handles;
    int64_t n;
    const uint8_t* keys;        /* INDEX */
    const int64_t* key_offsets; /* INDEX: n + 1 entries */
    int64_t key_bytes;          /* INDEX */
} tsq_dup_stream;
typedef struct tsq_dup_keys {   /* one stream's part of a push */
    const int64_t* handles;     /* HANDLE stream */
    const uint8_t* keys;        /* INDEX stream */
    const int64_t* key_offsets;
    int64_t key_bytes;
    const uint8_t* distinct;
} tsq_dup_keys;
typedef struct tsq_dup_conflict {
    int64_t row;
    int32_t stream;
    int32_t from_store;
    int64_t dup_handle;         /* from_store = 1 */
    int64_t dup_row;            /* from_store = 0; else -1 */
} tsq_dup_conflict;
typedef struct tsq_dup_result {
    int64_t affected, n_added, n_put, n_removed_store, n_removed_batch, rowid_base;
} tsq_dup_result;
typedef struct tsq_dupcheck tsq_dupcheck;
tsq_status tsq_dupcheck_create(tsq_ctx* ctx, const tsq_dup_stream* streams, int32_t n_streams, int32_t mode, const int64_t* table_handles,
                               int64_t n_table_rows, tsq_dupcheck** out);
tsq_status tsq_dupcheck_push(tsq_dupcheck* d, const tsq_dup_keys* keys, int32_t n_streams, int64_t n);
tsq_status tsq_dupcheck_match(tsq_dupcheck* d, tsq_dup_conflict* conflict, int64_t* cand_row, int64_t* cand_handle, int64_t* cand_ord,
                              int64_t* n_cand_batch, int64_t* n_cand_store);
tsq_status tsq_dupcheck_resolve(tsq_dupcheck* d, const uint8_t* equal_flags, int64_t rowid_base, uint8_t* added_out, uint8_t* put_out,
                                int64_t* handles_out, int64_t* removed_handles, int64_t* removed_ords, int64_t cap_removed,
                                tsq_dup_result* result);
/* forgets the statement's rows and verdict, keeps the store and every buffer: the next statement against the SAME store starts with its
 * first push (create copies and checks the whole store, which a statement of a few thousand rows should not pay again) */
tsq_status tsq_dupcheck_reset(tsq_dupcheck* d);
tsq_status tsq_dupcheck_stats(tsq_dupcheck* d, int64_t* rows, int64_t* pushes, int64_t* cand_batch, int64_t* cand_store, double* kernel_ms);
tsq_status tsq_dupcheck_cancel(tsq_dupcheck* d);
void       tsq_dupcheck_destroy(tsq_dupcheck* d);
/* types.EqualDatums over row pairs (types/datum.go:896-916, CompareDatum per column, types/compare.go:104-123): flags_out[i] (device,
 * one byte) = 1 iff row idx_a[i] of the columns cols_a equals row idx_b[i] of cols_b in every column: NULL equals NULL and nothing
 * else, integers by their 8 bytes, F32 / F64 with == (-0.0 equals 0.0, a NaN equals nothing, itself included), TSQ_BYTES by length and
 * bytes.  The two sides have the same n_cols (0..TSQ_MAX_COLS) and column types, device resident, null bitmaps allowed; idx_a / idx_b
 * are device arrays of n entries, or NULL for "pair i takes row i".  An index that is negative or beyond its side's rows gives 0. */
tsq_status tsq_rows_equal(tsq_ctx* ctx, const tsq_col* cols_a, const int64_t* idx_a, const tsq_col* cols_b, const int64_t* idx_b,
                          int32_t n_cols, int64_t n, uint8_t* flags_out);

/* ---------------------------------------------------------------- MVCC snapshot read: Scan, ReverseScan, Get
 * What tableScanExec.getRowFromRange / getRowFromPoint and indexScanExec ask of the store (store/mockstore/mocktikv/executor.go:124-189,
 * :271-320): mvccStore.Scan, ReverseScan and Get at the request's startTS (mvcc_leveldb.go:261-430).  The store is an immutable upload;
 * one upload serves readers at every startTS.
 *
 * THE STORE (tsq_mvcc_create, tsq_mvcc_data) is the reference's LevelDB content in its order, already decoded: n VERSIONS with their
 * raw user keys back to back (key_offsets: n + 1 entries into key_bytes bytes), keys ascending under bytes.Compare, the versions of
 * one key in descending commitTS; per version commit_ts, start_ts (uint64; start_ts is not read by any snapshot read and is not
 * kept, it may be NULL), its type (TSQ_MVCC_PUT / DELETE / ROLLBACK = typePut / typeDelete / typeRollback, mvcc.go:30-34) and its value
 * bytes (value_offsets: n + 1 entries).  LOCKS are a second list, at most one per key, keys ascending: startTS, ttl, the op
 * (TSQ_MVCC_OP_* = kvrpcpb.Op_Put / Del / Lock / Rollback) and the primary key's bytes.  A lock on a key without versions is legal: it
 * is a key of the store.  All arrays are host memory, or all device memory with data_flags = TSQ_COL_DEVICE; the library keeps its
 * own copy.  n = 0 and n_locks = 0 are legal.  n + n_locks >= 2^31: TSQ_ERR_UNSUPPORTED (decided before any array is read).  Everything else below is
 * TSQ_ERR_INVALID with the quoted tsq_last_error(ctx) text and no handle — checked by kernels, one lane per entry:
 *   "mvcc store: offsets decrease or leave their buffer" | "mvcc store: empty key" | "mvcc store: keys not ascending" |
 *   "mvcc store: versions of a key not descending in commitTS" (equal commitTS included: mvccEncode(key, ver) is a LevelDB key) |
 *   "mvcc store: a put with an empty value" (the reference's three read paths disagree about it: value != nil in Scan,
 *   len(val) == 0 in Get's callers, len(val) != 0 in finishEntry; no row or index entry has an empty value) |
 *   "mvcc store: value type or lock op out of range" | "mvcc store: lock keys not ascending" | "mvcc store: two locks on one key".
 * Create also builds what a read needs: a head flag and the key ordinal per version, the segment starts of the K keys that have
 * versions, each lock's place among them, and from those the KEY UNIVERSE — every distinct key with a version or a lock, with its
 * first version, its version count and its lock's index or -1.
 *
 * THE READ.  tsq_mvcc_scan answers Scan (desc = 0) or ReverseScan (desc = 1) range by range in the order given — the caller has
 * reversed the ranges for a descending scan, as reverseKVRanges does (cop_handler_dag.go:477-509).  Range r is host bytes
 * [start, end) = range_bytes[range_offsets[2r] .. [2r + 1]) and [.. [2r + 1] .. [2r + 2]); an empty start means from the first key, an
 * empty end to the last; start >= end selects nothing; ranges may overlap, each yields its own pairs.  range_flags[r] & TSQ_MVCC_POINT
 * (range_flags may be NULL): Get(start) — only the key equal to start, end is not read (getRowFromPoint).  Offsets that decrease or
 * leave range_bytes: TSQ_ERR_INVALID.  limit counts the pairs of all ranges together; limit < 0: no limit.
 * Per key exactly getValue (mvcc_leveldb.go:280-312): mvccLock.check (mvcc.go:197-207) — a lock with startTS > ts or op Op_Lock is
 * ignored; with ts = UINT64_MAX and the lock's primary equal to the key the key is read at lock.startTS - 1 (range scans and point
 * reads alike); any other lock is an error at that key — then the first version that is not a rollback and has commitTS <= ts decides:
 * a put yields the pair, a delete nothing, no such version nothing.  All timestamp comparisons are unsigned.  A descending scan yields
 * the same set per range in descending key order (mvccEntry.Get, mvcc.go:213-227, and finishEntry, mvcc_leveldb.go:418-430, reach
 * getValue's verdict on every store create accepts).
 * THE LOCK ERROR keeps the reference's order (the executors call the store with limit 1 and stop at the first error): the result is
 * the pairs in scan order across the ranges up to limit; a locked key met before limit pairs are complete makes the call answer
 * TSQ_ERR_LOCKED — whatever its versions say; one after the limit-th pair is never met.  result->n_pairs then counts the pairs before
 * it, nothing can be fetched, and tsq_mvcc_locked names it: the key, the lock's primary (host buffers; a too small one answers
 * TSQ_ERR_INVALID with the lengths filled in), startTS, ttl and op — ErrLocked's fields (mvcc.go:187-195; its Key is
 * mvccEncode(key, lockVer), built by the caller).  Without a preceding TSQ_ERR_LOCKED tsq_mvcc_locked answers TSQ_ERR_INVALID.
 * On TSQ_OK: result->n_pairs, key_bytes, value_bytes size the fetch; positions = the keys examined; range_counts (host, n_ranges
 * entries, may be NULL) = the pairs of every range after the limit (executor.go:76-85 Counts).
 * tsq_mvcc_fetch writes the pairs of the last scan into the caller's DEVICE buffers: keys back to back with n_pairs + 1 offsets, values
 * back to back with n_pairs + 1 offsets — what tsq_rowkeys_decode, tsq_rowcodec_decode and tsq_indexkeys_decode read.  key_cap <
 * key_bytes or value_cap < value_bytes: TSQ_ERR_INVALID, nothing is written.
 * A chain of TSQ_KNOB_MVCC_WAVE_CHAIN versions or more is walked by the whole wave, 64 versions per step.  A scan synchronises with
 * the host twice: once for the number of scan positions of its ranges (which sizes the per-position buffers), once for the counts
 * and the status.  Positions >= 2^31 (overlapping ranges): TSQ_ERR_UNSUPPORTED.
 * After tsq_mvcc_cancel every call answers TSQ_ERR_CANCELLED.  tsq_mvcc_stats: scans, keys examined, versions read, pairs returned
 * and the device time of the scans' kernels (two intervals per scan: the host's read of the position count between them is left out). */
#define TSQ_MVCC_PUT 0
#define TSQ_MVCC_DELETE 1
#define TSQ_MVCC_ROLLBACK 2
#define TSQ_MVCC_OP_PUT 0
#define TSQ_MVCC_OP_DEL 1
#define TSQ_MVCC_OP_LOCK 2
#define TSQ_MVCC_OP_ROLLBACK 3
#define TSQ_MVCC_POINT 1u
typedef struct tsq_mvcc_data {
    const uint8_t*  keys;
    const int64_t*  key_offsets;
    int64_t         key_bytes;
    const uint64_t* commit_ts;
    const uint64_t* start_ts;
    const uint8_t*  types;
    const uint8_t*  values;
    const int64_t*  value_offsets;
    int64_t         value_bytes;
    int64_t         n;
    const uint8_t*  lock_keys;
    const int64_t*  lock_key_offsets;
    int64_t         lock_key_bytes;
    const uint64_t* lock_start_ts;
    const uint64_t* lock_ttl;
    const uint8_t*  lock_ops;
    const uint8_t*  lock_primaries;
    const int64_t*  lock_primary_offsets;
    int64_t         lock_primary_bytes;
    int64_t         n_locks;
    uint32_t        data_flags;
    uint32_t        reserved;
} tsq_mvcc_data;
typedef struct tsq_mvcc_result {
    int64_t n_pairs;
    int64_t key_bytes;
    int64_t value_bytes;
    int64_t positions;
} tsq_mvcc_result;
typedef struct tsq_mvcc tsq_mvcc;
tsq_status tsq_mvcc_create(tsq_ctx* ctx, const tsq_mvcc_data* data, tsq_mvcc** out);
tsq_status tsq_mvcc_scan(tsq_mvcc* m, const uint8_t* range_bytes, const int64_t* range_offsets, const uint32_t* range_flags, int64_t n_ranges,
                         uint64_t start_ts, int32_t desc, int64_t limit, tsq_mvcc_result* result, int64_t* range_counts);
tsq_status tsq_mvcc_fetch(tsq_mvcc* m, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* values, int64_t value_cap,
                          int64_t* value_offsets);
tsq_status tsq_mvcc_locked(tsq_mvcc* m, uint8_t* key, int64_t key_cap, int64_t* key_len, uint8_t* primary, int64_t primary_cap,
                           int64_t* primary_len, uint64_t* start_ts, uint64_t* ttl, int32_t* op);
tsq_status tsq_mvcc_stats(tsq_mvcc* m, int64_t* scans, int64_t* keys_examined, int64_t* versions_read, int64_t* pairs, double* kernel_ms);
tsq_status tsq_mvcc_cancel(tsq_mvcc* m);
void       tsq_mvcc_destroy(tsq_mvcc* m);

/* ---------------------------------------------------------------- MVCC writes: Prewrite, Commit, Rollback into the next store
 * The two-phase-commit write calls of the reference's MVCCLevelDB (store/mockstore/mocktikv/mvcc_leveldb.go: Prewrite :442-537,
 * Commit :540-613, Rollback :616-700 with getTxnCommitInfo :702-717), applied to a store in HBM.  A store stays IMMUTABLE: a write that
 * succeeds returns a new handle, the NEXT STORE, and leaves the handle it was called on untouched and readable — readers at any
 * startTS keep their snapshot; the caller destroys the old handle when it is done with it.  A write that meets an error writes
 * nothing and returns no handle, as the reference drops its LevelDB batch.  The next store is a full rewrite of the arrays (no delta
 * layer): one stream over the store plus O(keys * log U) for the verdicts.
 *
 * A WRITABLE STORE comes from tsq_mvcc_create_rw: tsq_mvcc_create plus the value of every lock (lock_values back to back,
 * lock_value_offsets: n_locks + 1 entries; host or device like the rest of `data`), which a commit turns into the version's value.
 * data->start_ts is required (n > 0) and kept.  Beyond the checks of tsq_mvcc_create: "mvcc store: a put lock with an empty value" and the
 * offsets message for lock_value_offsets.  Reads on a writable store behave exactly as on a plain one.  The write calls on a store
 * from plain tsq_mvcc_create answer TSQ_ERR_INVALID "mvcc write: the store was created without start_ts and lock values (tsq_mvcc_create_rw)".
 *
 * THE REQUEST (tsq_mvcc_write_req): n_keys raw keys back to back (key_offsets: n_keys + 1 entries into key_bytes bytes); Prewrite
 * also takes per key ops (TSQ_MVCC_OP_PUT / DEL / LOCK) and values (value_offsets: n_keys + 1 entries into value_bytes bytes), and
 * the primary key (host bytes always), startTS and ttl; Commit reads start_ts and commit_ts, Rollback start_ts.  The arrays are all
 * host memory, or all device memory with flags = TSQ_COL_DEVICE.  n_keys = 0 is legal: the next store equals the current one.
 * "Chain" below: the versions of one key in descending commitTS, rollbacks included.  All timestamp comparisons are unsigned.
 *
 * PREWRITE (prewriteMutation :493-537).  Each mutation's verdict is independent of the other mutations of the request — the
 * reference reads db, not the pending batch (:497).  A lock on the key with lock.startTS != startTS: TSQ_MVCC_V_LOCKED (:509-512;
 * lockErr's fields through tsq_mvcc_lock_at).  A lock with lock.startTS == startTS: OK, the lock is replaced and the conflict check
 * is not run (:509-518).  No lock: the newest entry of the chain decides, whatever its type, rollbacks included (:481-489): commitTS >=
 * startTS is TSQ_MVCC_V_CONFLICT with ConflictTS = that version's start_ts and ConflictCommitTS = its commit_ts.  A key without
 * versions has commitTS 0, so it conflicts exactly when startTS == 0, with both fields 0.  Otherwise OK.  Every mutation gets its
 * verdict, as Prewrite returns one error per mutation (:452-461); if any is an error nothing is written (:462-464), otherwise every key
 * gets the lock {startTS, primary, value, op, ttl} (:520-535).
 * COMMIT (commitKey :556-588).  A lock with lock.startTS == startTS is committed (commitLock :590-613): op != Op_Lock adds the version
 * (PUT if op == Op_Put else DELETE, startTS, commitTS, lock.value), replacing a version with the same (key, commitTS) — one LevelDB
 * key (:604) — and the lock is removed (:611).  Otherwise the first version of the chain with start_ts == startTS (:573, :702-717): it
 * exists and is not a rollback: TSQ_MVCC_V_NOOP (:577-580); else TSQ_MVCC_V_TXN_NOT_FOUND (:581).  The reference stops at the first
 * failing key (:547-552); here every key gets a verdict and first_error names the reference's error.
 * ROLLBACK (rollbackKey :632-684).  The own lock: it is removed and (ROLLBACK, startTS, commitTS = startTS, empty value) is added,
 * replacing an equal (key, startTS) version (:648-653, :686-700).  Otherwise the first version with start_ts == startTS (:657): not a
 * rollback: TSQ_MVCC_V_ALREADY_COMMITTED with its commitTS (:663-665); a rollback: TSQ_MVCC_V_NOOP (:666-667); none: the rollback
 * version is added, a foreign lock on the key stays (:671-683).
 *
 * DEPARTURES.  The keys of a request must be strictly ascending (the two-phase committer walks the transaction's sorted buffer; the
 * apply is a merge of two sorted lists): TSQ_ERR_INVALID "mvcc write: keys not strictly ascending".  Refused with TSQ_ERR_INVALID,
 * checked by a kernel, one lane per key: "mvcc write: empty key" | "mvcc write: offsets decrease or leave their buffer" |
 * "mvcc write: a prewrite op other than Put, Del or Lock" | "mvcc write: a put with an empty value"; and by the host:
 * "mvcc write: commitTS 2^64 - 1 is the lock's version" (a commit at UINT64_MAX, a rollback at startTS UINT64_MAX).
 * n + n_locks + n_keys >= 2^31: TSQ_ERR_UNSUPPORTED "mvcc write: 2^31 entries or more", before any array is read.
 *
 * OUTPUTS (host memory, n_keys entries; may be NULL): verdicts, one byte per key (TSQ_MVCC_V_*); info, two uint64 per key:
 * LOCKED: the lock's index, 0; CONFLICT: ConflictTS, ConflictCommitTS; ALREADY_COMMITTED: the commitTS, 0; otherwise 0, 0.
 * result: n_errors (verdicts >= TSQ_MVCC_V_LOCKED), first_error (the smallest key index with an error, -1: none), versions_added
 * (new versions, those that replace one included), versions_replaced, locks_added (a replaced lock counts as added and removed),
 * locks_removed, kernel_ms (device time of the verdict and apply passes).  The call answers TSQ_OK and *next is set iff n_errors == 0;
 * with errors *next = NULL and the store is as it was.  The next store is writable; cancel and destroy work on it like on any other.
 * Its head flags, ordinals and universe come from the create kernels over the new arrays, and their checks run on it as an internal
 * assertion: a failure there is TSQ_ERR_HIP "internal: ...", never a damaged handle.  A call that fails or reports errors leaves no
 * handle and no device memory behind.
 * tsq_mvcc_lock_at: the fields of lock j in the buffer convention of tsq_mvcc_locked — for the LOCKED verdicts.
 * tsq_mvcc_sizes / tsq_mvcc_export: the counts and byte sizes of a writable store, then every array of it into the caller's DEVICE
 * buffers (tsq_mvcc_arrays; a NULL member is skipped; offsets arrays have count + 1 entries): versions with start_ts, locks with
 * values — reads cannot see rollback versions, start_ts or lock fields; a caller persists a store with it. */
#define TSQ_MVCC_V_OK 0
#define TSQ_MVCC_V_NOOP 1
#define TSQ_MVCC_V_LOCKED 2
#define TSQ_MVCC_V_CONFLICT 3
#define TSQ_MVCC_V_TXN_NOT_FOUND 4
#define TSQ_MVCC_V_ALREADY_COMMITTED 5
typedef struct tsq_mvcc_write_req {
    const uint8_t*  keys;
    const int64_t*  key_offsets;
    int64_t         key_bytes;
    int64_t         n_keys;
    const uint8_t*  ops;
    const uint8_t*  values;
    const int64_t*  value_offsets;
    int64_t         value_bytes;
    const uint8_t*  primary;
    int64_t         primary_len;
    uint64_t        start_ts;
    uint64_t        commit_ts;
    uint64_t        ttl;
    uint32_t        flags;
    uint32_t        reserved;
} tsq_mvcc_write_req;
typedef struct tsq_mvcc_write_result {
    int64_t n_errors;
    int64_t first_error;
    int64_t versions_added;
    int64_t versions_replaced;
    int64_t locks_added;
    int64_t locks_removed;
    double  kernel_ms;
} tsq_mvcc_write_result;
typedef struct tsq_mvcc_store_sizes {
    int64_t n;
    int64_t n_locks;
    int64_t key_bytes;
    int64_t value_bytes;
    int64_t lock_key_bytes;
    int64_t lock_primary_bytes;
    int64_t lock_value_bytes;
} tsq_mvcc_store_sizes;
typedef struct tsq_mvcc_arrays {
    uint8_t*  keys;
    int64_t*  key_offsets;
    uint64_t* commit_ts;
    uint64_t* start_ts;
    uint8_t*  types;
    uint8_t*  values;
    int64_t*  value_offsets;
    uint8_t*  lock_keys;
    int64_t*  lock_key_offsets;
    uint64_t* lock_start_ts;
    uint64_t* lock_ttl;
    uint8_t*  lock_ops;
    uint8_t*  lock_primaries;
    int64_t*  lock_primary_offsets;
    uint8_t*  lock_values;
    int64_t*  lock_value_offsets;
} tsq_mvcc_arrays;
tsq_status tsq_mvcc_create_rw(tsq_ctx* ctx, const tsq_mvcc_data* data, const uint8_t* lock_values, const int64_t* lock_value_offsets,
                              int64_t lock_value_bytes, tsq_mvcc** out);
tsq_status tsq_mvcc_prewrite(tsq_mvcc* m, const tsq_mvcc_write_req* req, uint8_t* verdicts, uint64_t* info, tsq_mvcc_write_result* result,
                             tsq_mvcc** next);
tsq_status tsq_mvcc_commit(tsq_mvcc* m, const tsq_mvcc_write_req* req, uint8_t* verdicts, uint64_t* info, tsq_mvcc_write_result* result,
                           tsq_mvcc** next);
tsq_status tsq_mvcc_rollback(tsq_mvcc* m, const tsq_mvcc_write_req* req, uint8_t* verdicts, uint64_t* info, tsq_mvcc_write_result* result,
                             tsq_mvcc** next);
tsq_status tsq_mvcc_lock_at(tsq_mvcc* m, int64_t j, uint8_t* key, int64_t key_cap, int64_t* key_len, uint8_t* primary, int64_t primary_cap,
                            int64_t* primary_len, uint64_t* start_ts, uint64_t* ttl, int32_t* op);
tsq_status tsq_mvcc_sizes(tsq_mvcc* m, tsq_mvcc_store_sizes* out);
tsq_status tsq_mvcc_export(tsq_mvcc* m, const tsq_mvcc_arrays* out);

/* ---------------------------------------------------------------- MVCC lock resolution and GC: ScanLock, ResolveLock, GC, DeleteRange
 * The range calls of the reference's MVCCLevelDB (store/mockstore/mocktikv/mvcc_leveldb.go: ScanLock :906-939, ResolveLock :942-978,
 * BatchResolveLock :981-1019, GC :1022-1085, DeleteRange :1088-1090) over a store in HBM (addition to ABI 10: nothing existing changes
 * shape).  Each is one pass over a key range with one decision per lock or per version.  The handle model is the writes': the store is
 * immutable; a call that changes something returns the NEXT STORE as a new writable handle in *next and leaves the handle it was
 * called on untouched and readable.
 *
 * THE RANGE [start, end) is host bytes with newScanIterator's meaning (:149-171), as tsq_mvcc_scan's: an empty start is the first key,
 * an empty end the last one, start >= end selects nothing.  DEPARTURE FOR tsq_mvcc_delete_range ALONE: the reference compares
 * EncodeBytes(start) and EncodeBytes(end) as raw LevelDB bounds (:1088-1090, doRawDeleteRange :1231-1246), and no stored key sorts
 * under EncodeBytes("") — there an EMPTY END DELETES NOTHING (an empty start is still the first key).
 *
 * CHANGED NOTHING.  A mutating call that changes nothing — no lock matched, nothing at or under the safe point, an empty range —
 * answers TSQ_OK with *next = NULL and all counts zero: the store is its own successor and no rewrite is paid for.
 *
 * tsq_mvcc_scan_lock (any store, plain or writable): the locks of the range with start_ts <= max_ts (:923), in key order.  result:
 * n_locks and the byte sizes of their keys and primaries, which size tsq_mvcc_scan_lock_fetch: keys back to back with n_locks + 1
 * offsets, primaries back to back with n_locks + 1 offsets, start_ts and lock_index (the lock's index among the store's sorted lock
 * keys, what tsq_mvcc_lock_at takes), n_locks entries each — LockInfo{PrimaryLock, LockVersion, Key} per lock.  The buffers are host
 * memory, or all device memory with flags = TSQ_COL_DEVICE.  key_cap < key_bytes or primary_cap < primary_bytes: TSQ_ERR_INVALID,
 * nothing is written.  Without a preceding successful tsq_mvcc_scan_lock the fetch answers TSQ_ERR_INVALID.
 *
 * tsq_mvcc_resolve_lock (writable stores): n_txns pairs (txn_start_ts[i], txn_commit_ts[i]), host arrays in any order — n_txns == 1
 * is ResolveLock, more is BatchResolveLock's map; a start_ts given twice is TSQ_ERR_INVALID "mvcc resolve lock: a start_ts given
 * twice".  Every lock of the range whose start_ts is in the list is resolved.  commit_ts > 0: commitLock (:590-613) — op != Op_Lock adds
 * the version (PUT if op == Op_Put else DELETE, the lock's start_ts, commit_ts, the lock's value), replacing a version with an equal
 * (key, commitTS); the lock goes.  commit_ts == 0: rollbackLock (:686-700) — (ROLLBACK, start_ts, commitTS = start_ts, empty value) is
 * added, replacing an equal (key, start_ts) version; the lock goes.  There are no verdicts: the reference checks nothing here.  A
 * commit_ts of UINT64_MAX and a rollback at start_ts UINT64_MAX are TSQ_ERR_INVALID "mvcc resolve lock: commitTS 2^64 - 1 is the
 * lock's version".  n + 2 n_locks >= 2^31 (every lock may add a version): TSQ_ERR_UNSUPPORTED before any array is read.
 *
 * tsq_mvcc_gc (writable stores): if any lock of the range has start_ts <= safe_point nothing is written (:1041-1047): result->n_errors
 * counts those locks, first_error is the index of the first of them in key order (for tsq_mvcc_lock_at), *next = NULL, TSQ_OK.
 * Otherwise per key of the range, over its versions in descending commitTS (:1052-1080): a version with commit_ts > safe_point stays;
 * of the rest every ROLLBACK goes, the first PUT-or-DELETE stays iff it is a PUT, every later PUT or DELETE goes.  A key that loses
 * every version and has no lock leaves the store's key universe.
 *
 * tsq_mvcc_delete_range (writable stores): every version and the lock of every key with start <= key < end go (see the departure above).
 *
 * result (tsq_mvcc_maint_result): versions_added (those that replace one included), versions_replaced, versions_removed (GC,
 * DeleteRange), locks_removed, n_errors / first_error (GC's refusal; -1: none), kernel_ms (device time of all passes), mark_ms (of
 * the bound and marking passes alone, the part in front of the apply).  A plain store answers the three mutating calls with
 * TSQ_ERR_INVALID "...: the store was created without start_ts and lock values (tsq_mvcc_create_rw)".  The limits and failure rules
 * of the writes hold: a failed or refused call leaves no handle and no device memory behind; after tsq_mvcc_cancel every call answers
 * TSQ_ERR_CANCELLED; the next store's head flags, ordinals and universe come from the create kernels, their checks being the
 * internal assertion. */
typedef struct tsq_mvcc_lock_scan {
    int64_t n_locks;
    int64_t key_bytes;
    int64_t primary_bytes;
    double  kernel_ms;
} tsq_mvcc_lock_scan;
typedef struct tsq_mvcc_maint_result {
    int64_t versions_added;
    int64_t versions_replaced;
    int64_t versions_removed;
    int64_t locks_removed;
    int64_t n_errors;
    int64_t first_error;
    double  kernel_ms;
    double  mark_ms;
} tsq_mvcc_maint_result;
tsq_status tsq_mvcc_scan_lock(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len, uint64_t max_ts,
                              tsq_mvcc_lock_scan* result);
tsq_status tsq_mvcc_scan_lock_fetch(tsq_mvcc* m, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* primaries, int64_t primary_cap,
                                    int64_t* primary_offsets, uint64_t* start_ts, int64_t* lock_index, uint32_t flags);
tsq_status tsq_mvcc_resolve_lock(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len,
                                 const uint64_t* txn_start_ts, const uint64_t* txn_commit_ts, int64_t n_txns, tsq_mvcc_maint_result* result,
                                 tsq_mvcc** next);
tsq_status tsq_mvcc_gc(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len, uint64_t safe_point,
                       tsq_mvcc_maint_result* result, tsq_mvcc** next);
tsq_status tsq_mvcc_delete_range(tsq_mvcc* m, const uint8_t* start, int64_t start_len, const uint8_t* end, int64_t end_len,
                                 tsq_mvcc_maint_result* result, tsq_mvcc** next);

/* ---------------------------------------------------------------- Transaction buffer: sorted mutations of one transaction
 * The reference's write buffer, kv.memDbBuffer (kv/memdb_buffer.go:95-114: Set, Delete = a put of an empty value) as
 * twoPhaseCommitter.initKeysAndMutations walks it (store/tikv/2pc.go:115-172), in HBM (addition to ABI 10: nothing existing changes
 * shape): an ordered map from byte keys to values.  The last write to a key wins, an empty value becomes Op_Del, and a key of
 * tikvTxn.LockKeys becomes Op_Lock only if nothing else wrote it (:159-171).  What comes out is a tsq_mvcc_write_req whose keys are
 * strictly ascending — the form the MVCC writes ask for — without a key or value byte crossing to the host.
 *
 * tsq_membuf_push: n entries of one kind (TSQ_MEMBUF_SET / DELETE / LOCK) are COPIED into the buffer — the caller may free its
 * batch when the call returns; host arrays, or all device arrays with data_flags = TSQ_COL_DEVICE.  key_offsets: n + 1 entries into
 * key_bytes bytes, or NULL for keys of one fixed length key_bytes / n (record keys arrive that way; key_bytes must then be a
 * multiple of n).  values / value_offsets / value_bytes are read for SET only.  Every entry gets a SEQUENCE NUMBER: push order, then
 * row order inside a push.  Refused with TSQ_ERR_INVALID and *error_row = the first such row (-1 otherwise), checked by a kernel, one lane per row;
 * the push then adds NOTHING: "membuf: empty key" (as the prewrite refuses it) | "membuf: cannot set nil value" (ErrCannotSetNilValue,
 * memdb_buffer.go:96) | "membuf: entry too large" (ErrEntryTooLarge, :99: a SET with len(k) + len(v) > entry_size_limit) |
 * "membuf: offsets decrease or leave their buffer".  PINNED DEPARTURE: the reference has already stored the rows in front of the
 * failing one; the statement fails either way.  Limit: fewer than 2^31 pushed entries, TSQ_ERR_UNSUPPORTED beyond.
 *
 * tsq_membuf_finish: orders the entries by bytes.Compare (memcmp over the common length, then the shorter key first); among equal
 * keys only the entry with the largest sequence number stays, except that a LOCK entry loses to any SET or DELETE of the same key
 * whatever the order, and duplicate lock keys collapse.  Survivors become TSQ_MVCC_OP_PUT / DEL / LOCK.  result: n_entries, puts,
 * dels, locks, size (the sum of len(k) + len(v) over the survivors = c.txnSize), primary_index (the reference's c.keys[0],
 * 2pc.go:211-214: the smallest key that is not lock-only; if there is none the first lock key pushed; -1 for an empty buffer),
 * sort_passes (radix passes run; 0 when the entries arrived strictly ascending), kernel_ms.  size > total_size_limit:
 * TSQ_ERR_INVALID "membuf: transaction too large" (ErrTxnTooLarge).  PINNED DEPARTURE: the reference checks the running size after
 * every Set; here the final size is checked once.  Calling finish again after more pushes gives what one finish over all pushes
 * would give (the sort is redone).  A limit of 0 means none.
 *
 * tsq_membuf_request: after a finish, fills a tsq_mvcc_write_req with the buffer's own DEVICE arrays (keys, key_offsets, ops,
 * values, value_offsets, the counts, flags = TSQ_COL_DEVICE); primary / primary_len / start_ts / commit_ts / ttl are left zero for
 * the caller.  The arrays pass tsq_mvcc_prewrite / commit / rollback as they are and stay valid until the next push or destroy.
 * tsq_membuf_get: batched memDbBuffer.Get after a finish — entry_out[i] (host, n entries) = the index of key i among the request's
 * entries, -1 = ErrNotExist; a deleted key is found (its op is TSQ_MVCC_OP_DEL); a LOCK-ONLY key answers -1, as the reference keeps
 * lock keys beside the buffer, not in it.  Keys as in a push.  Before a finish, or after a push that followed it: TSQ_ERR_INVALID
 * "membuf: not finished".
 * kernel_ms is stream time, not a sum of kernels: the survey, then from the first pass to the last copy with the host's reads of the
 * control words in between. */
typedef struct tsq_membuf_cfg {
    int64_t  entry_size_limit;   /* kv.TxnEntrySizeLimit; 0 = none */
    int64_t  total_size_limit;   /* kv.TxnTotalSizeLimit; 0 = none */
    uint32_t flags;
    uint32_t reserved;
} tsq_membuf_cfg;
#define TSQ_MEMBUF_SET 0      /* memDbBuffer.Set    */
#define TSQ_MEMBUF_DELETE 1   /* memDbBuffer.Delete */
#define TSQ_MEMBUF_LOCK 2     /* tikvTxn.LockKeys   */
typedef struct tsq_membuf_result {
    int64_t n_entries;
    int64_t puts;
    int64_t dels;
    int64_t locks;
    int64_t size;
    int64_t primary_index;
    int64_t sort_passes;
    double  kernel_ms;
} tsq_membuf_result;
typedef struct tsq_membuf tsq_membuf;
tsq_status tsq_membuf_create(tsq_ctx* ctx, const tsq_membuf_cfg* cfg, tsq_membuf** out);
tsq_status tsq_membuf_push(tsq_membuf* mb, int32_t kind, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n,
                           const uint8_t* values, const int64_t* value_offsets, int64_t value_bytes, uint32_t data_flags, int64_t* error_row);
tsq_status tsq_membuf_finish(tsq_membuf* mb, tsq_membuf_result* result);
tsq_status tsq_membuf_request(tsq_membuf* mb, tsq_mvcc_write_req* req);
tsq_status tsq_membuf_get(tsq_membuf* mb, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n, uint32_t data_flags,
                          int64_t* entry_out);
void       tsq_membuf_destroy(tsq_membuf* mb);

/* ---------------------------------------------------------------- Transaction buffer: mem readers and dirty handles (DESIGN.md §5 "Mem readers")
 * Read your own writes (addition to ABI 10: nothing existing changes shape): what executor/mem_reader.go builds on the host for a
 * statement that reads a table its own transaction has written — iterTxnMemBuffer (:256-281) over memDbBuffer.Iter
 * (kv/memdb_buffer.go:51-65, Valid :142-147) — over the arrays the last tsq_membuf_finish left, without a key or value byte leaving
 * the device; and the two handle sets of executor.DirtyTable (union_scan.go:56-74) read out of the same buffer.
 *
 * tsq_membuf_scan: ranges laid out as tsq_mvcc_scan's — range r = [start, end) = range_bytes[range_offsets[2r] .. [2r + 1]) and
 * [.. [2r + 1] .. [2r + 2]), 2 * n_ranges + 1 offsets; host arrays, or all device arrays with data_flags = TSQ_COL_DEVICE.  A range
 * selects the entries whose key k has start <= k < end under bytes.Compare; an empty start means from the first key; start >= end
 * selects nothing; ranges may overlap, each yields its own pairs, in the order given.  Of the selected entries only the
 * TSQ_MVCC_OP_PUT ones yield a pair: a DEL is the reference's len(iter.Value()) == 0, a lock-only key is not in the reference's
 * buffer at all.  desc = 1 gives the WHOLE sequence reversed — reverseDatumSlice over the rows of all ranges (mem_reader.go:129-131),
 * not range by range.  result: n_pairs, key_bytes and value_bytes (which size the fetch), positions (the entries examined, over all
 * ranges) and skipped_dels; range_counts (host, n_ranges entries, may be NULL): the pairs of every range.  n_ranges = 0 and an empty
 * buffer are legal and answer zero pairs.  Before a finish, or after a push that followed it: TSQ_ERR_INVALID "membuf: not finished",
 * as tsq_membuf_get; offsets that decrease or leave their buffer: TSQ_ERR_INVALID; 2^31 positions or more: TSQ_ERR_UNSUPPORTED.
 * PINNED DEPARTURE: the C-ABI cannot tell a nil bound from an empty one — an empty end means "to the last key", as in tsq_mvcc_scan;
 * the reference's empty non-nil upperBound selects nothing; the mem readers never pass one.
 * tsq_membuf_scan_points: n keys passed as in a push (key_offsets NULL: keys of key_bytes / n bytes each, how record keys arrive).
 * Key i yields its pair iff the buffer holds it as a PUT; input order is kept and a repeated key yields its pair each time — what
 * memIndexLookUpReader.getMemRows asks for (mem_reader.go:359-398): one [key(h), key(h).PrefixNext()) range per handle, in the
 * index's order.  positions counts the keys the buffer holds (PUT, DEL or lock-only).
 * tsq_membuf_fetch: writes the pairs of the last scan (of either kind) into the caller's DEVICE buffers in exactly the form
 * tsq_mvcc_fetch writes — keys back to back with n_pairs + 1 offsets, values back to back with n_pairs + 1 offsets — which
 * tsq_rowkeys_decode, tsq_rowcodec_decode and tsq_indexkeys_decode read unchanged.  key_cap < key_bytes or value_cap < value_bytes:
 * TSQ_ERR_INVALID, nothing is written.  Without a preceding successful scan (or after a push or finish that followed it):
 * TSQ_ERR_INVALID.  A scan synchronises with the host twice: once for the position total (which sizes the per-position buffers),
 * once for the counts and the status.
 *
 * tsq_membuf_dirty: one pass over the entries inside ['t' | EncodeInt(table_id) | "_r", 't' | EncodeInt(table_id) | "_s"): a PUT's
 * handle (decoded as tsq_rowkeys_decode does) goes to the added list, a DEL's to the deleted list, a lock-only key to neither; a key
 * in that range that is not 19 bytes long: TSQ_ERR_INVALID "invalid key".  tsq_membuf_dirty_fetch writes both lists to DEVICE
 * buffers of n_added and n_deleted entries (either may be NULL when its count is 0), each ascending as signed int64: they fall out
 * in key order.  PINNED DEPARTURE, invisible to UnionScan: DirtyTable is fed per statement, so a handle deleted and then
 * re-inserted is in both of its sets; here it is in `added` only.  getSnapshotRow (union_scan.go:212-220) drops a snapshot row whose
 * handle is in EITHER set, so only the union matters, and the union is exactly the record keys the buffer holds for the table:
 * AddRecord and RemoveRecord write the record key whenever they touch DirtyTable. */
typedef struct tsq_membuf_scan_result {
    int64_t n_pairs;
    int64_t key_bytes;
    int64_t value_bytes;
    int64_t positions;
    int64_t skipped_dels;
} tsq_membuf_scan_result;
tsq_status tsq_membuf_scan(tsq_membuf* mb, const uint8_t* range_bytes, const int64_t* range_offsets, int64_t n_ranges, uint32_t data_flags,
                           int32_t desc, tsq_membuf_scan_result* result, int64_t* range_counts);
tsq_status tsq_membuf_scan_points(tsq_membuf* mb, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n,
                                  uint32_t data_flags, tsq_membuf_scan_result* result);
tsq_status tsq_membuf_fetch(tsq_membuf* mb, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* values, int64_t value_cap,
                            int64_t* value_offsets);
tsq_status tsq_membuf_dirty(tsq_membuf* mb, int64_t table_id, int64_t* n_added, int64_t* n_deleted);
tsq_status tsq_membuf_dirty_fetch(tsq_membuf* mb, int64_t* added_out, int64_t* deleted_out);

/* ---------------------------------------------------------------- UnionStore: a transaction's reads over buffer and snapshot (DESIGN.md §5 "UnionStore")
 * The KV-level merge every read of a transaction goes through (addition to ABI 10: nothing existing changes shape): BufferStore.Get
 * (kv/buffer_store.go:61-73) and BufferStore.Iter / IterReverse, which build a kv.UnionIter (kv/union_iter.go:64-152), over a finished
 * tsq_membuf as the dirty side and a tsq_mvcc store read at start_ts as the snapshot side.  tsq_unionstore_create BORROWS both
 * handles: destroying the store or the buffer before the union store is the caller's error.  mb may be NULL — lazyMemBuffer never
 * written: every read is then the snapshot's.
 *
 * The dirty side is the finished buffer's TSQ_MVCC_OP_PUT and TSQ_MVCC_OP_DEL entries; a lock-only key is not in the reference's
 * memDbBuffer and shadows nothing.  The snapshot side is what tsq_mvcc_scan resolves at start_ts: getValue, the lock check and the
 * UINT64_MAX / primary rule, unchanged.
 *
 * tsq_unionstore_scan: ranges laid out as tsq_mvcc_scan's, [start, end) each (no point flags); host arrays, or all device arrays with
 * data_flags = TSQ_COL_DEVICE.  An empty start means from the first key, an empty end to the last, start >= end selects nothing;
 * ranges may overlap, each yields its own pairs in the order given.  Per range, keys compared by bytes.Compare: a buffer PUT yields
 * (key, buffer value), a buffer DEL yields nothing, in both cases a snapshot pair of the same key is dropped; a snapshot pair whose
 * key the buffer does not hold as PUT or DEL is yielded as it is.  desc = 1: every range comes out descending, range by range — this
 * is tsq_mvcc_scan's convention, NOT tsq_membuf_scan's reversal of the whole sequence.  limit counts the pairs of all ranges together
 * (limit < 0: none; limit = 0 answers zero pairs and examines nothing); range_counts (host, n_ranges entries, may be NULL) is per
 * range after the limit.  result: n_pairs, key_bytes and value_bytes (which size the fetch); positions_snapshot and positions_buffer
 * (the keys either side examined, over all ranges); shadowed (the visible snapshot pairs a buffer PUT or DEL replaced), skipped_dels
 * (the DELs inside the ranges), dangling_dels (the DELs with no visible snapshot pair: the reference's "delete a record not exists?"
 * warning, counted instead of logged) — these three over everything the ranges select, whatever the limit; from_buffer (the returned
 * pairs that come from the buffer).
 * THE LOCK ERROR keeps the reference's order.  The snapshot iterator (store/tikv/scan.go:88-135) fails when it steps onto a locked
 * key; UnionIter steps it at construction, on Next after a snapshot pair was yielded, and inside updateCur as soon as a buffer key
 * equals the snapshot key (union_iter.go:98-115) — so a locked key is met even where the buffer would have shadowed it, and the
 * buffer's own pair of the key in front of it is not yielded first.  The consumer takes pairs while Valid() and fewer than limit are
 * taken, does not call Next after the limit-th pair, and opens a range only while the limit is not reached.  On a met lock the call
 * answers TSQ_ERR_LOCKED, n_pairs is the pairs taken before it, nothing can be fetched, and tsq_unionstore_locked names the lock with
 * the fields and buffer rules of tsq_mvcc_locked.
 * tsq_unionstore_get: n keys passed as in a push (key_offsets NULL: keys of key_bytes / n bytes each), one verdict per key in input
 * order: a buffer PUT gives its value; a buffer DEL gives ErrNotExist WITHOUT reading the snapshot (a lock on that key is not met);
 * every other key goes to the snapshot's Get: a pair, ErrNotExist, or the lock error — the first key in input order that meets a lock
 * fails the call.  A repeated key is answered each time.  found (host, n bytes, may be NULL): 1 where key i has a pair; the pairs
 * of the found keys, in input order, are what the fetch writes.
 * tsq_unionstore_fetch: the pairs of the last scan or get into the caller's DEVICE buffers, in exactly the form tsq_mvcc_fetch and
 * tsq_membuf_fetch write, which tsq_rowkeys_decode, tsq_rowcodec_decode and tsq_indexkeys_decode read unchanged; from_buffer (device,
 * n_pairs bytes, may be NULL): UnionIter's curIsDirty of every pair.  Too small a buffer: TSQ_ERR_INVALID, nothing is written.
 * A buffer that is not finished — or was pushed to or finished again since the scan, for a fetch — answers TSQ_ERR_INVALID
 * "membuf: not finished", as tsq_membuf_scan does.  Offsets that decrease or leave their buffer: TSQ_ERR_INVALID; 2^31 positions of
 * both sides together or more: TSQ_ERR_UNSUPPORTED.
 * ROUTES (tsq_unionstore_stats names the last one).  TSQ_UNION_ROUTE_SNAPSHOT: mb is NULL or empty, n_ranges or limit is 0, or no range holds a buffer entry
 * — the read IS tsq_mvcc_scan + tsq_mvcc_fetch on the borrowed store (whose last scan it replaces), pair for pair.
 * TSQ_UNION_ROUTE_MERGE: both sides' positions are placed among their range's candidates by one bound search each.
 * TSQ_UNION_ROUTE_POINTS: a get.  On the snapshot route the pairs are the borrowed store's last scan: a tsq_mvcc_scan of the store by
 * anyone else between this handle's scan and its fetch (or its tsq_unionstore_locked) takes their place, and the fetch answers
 * TSQ_ERR_INVALID "the store was scanned since this handle's read".
 * HOST SYNCHRONISATIONS.  A merged scan two (the position totals, which size the per-position buffers; the counts and the status);
 * a get one; a snapshot-route scan tsq_mvcc_scan's two, plus one when the buffer's bounds had to be searched first (a non-empty
 * buffer none of whose entries the ranges hold: the bound pass then runs twice, here and in tsq_mvcc_scan).  Ranges passed as
 * TSQ_COL_DEVICE cost more: their offsets are read back with a blocking copy before anything else (one more synchronisation on
 * either route), and on the snapshot route their bytes too (another one) — tsq_mvcc_scan takes host ranges and uploads them again.
 * A caller that has its ranges on the host should pass them from there. */
#define TSQ_UNION_ROUTE_NONE 0
#define TSQ_UNION_ROUTE_MERGE 1
#define TSQ_UNION_ROUTE_SNAPSHOT 2
#define TSQ_UNION_ROUTE_POINTS 3
typedef struct tsq_unionstore tsq_unionstore;
typedef struct tsq_unionstore_result {
    int64_t n_pairs;
    int64_t key_bytes;
    int64_t value_bytes;
    int64_t positions_snapshot;
    int64_t positions_buffer;
    int64_t shadowed;
    int64_t skipped_dels;
    int64_t dangling_dels;
    int64_t from_buffer;
} tsq_unionstore_result;
tsq_status tsq_unionstore_create(tsq_ctx* ctx, tsq_mvcc* store, tsq_membuf* mb, uint64_t start_ts, tsq_unionstore** out);
tsq_status tsq_unionstore_scan(tsq_unionstore* us, const uint8_t* range_bytes, const int64_t* range_offsets, int64_t n_ranges, uint32_t data_flags,
                               int32_t desc, int64_t limit, tsq_unionstore_result* result, int64_t* range_counts);
tsq_status tsq_unionstore_get(tsq_unionstore* us, const uint8_t* keys, const int64_t* key_offsets, int64_t key_bytes, int64_t n, uint32_t data_flags,
                              tsq_unionstore_result* result, uint8_t* found);
tsq_status tsq_unionstore_fetch(tsq_unionstore* us, uint8_t* keys, int64_t key_cap, int64_t* key_offsets, uint8_t* values, int64_t value_cap,
                                int64_t* value_offsets, uint8_t* from_buffer);
tsq_status tsq_unionstore_locked(tsq_unionstore* us, uint8_t* key, int64_t key_cap, int64_t* key_len, uint8_t* primary, int64_t primary_cap,
                                 int64_t* primary_len, uint64_t* start_ts, uint64_t* ttl, int32_t* op);
/* scans of either route, merged scans, snapshot-route scans, gets, pairs returned, the route of the last read, device time of the
 * merged scans and gets (the snapshot route's is in tsq_mvcc_stats) */
tsq_status tsq_unionstore_stats(tsq_unionstore* us, int64_t* scans, int64_t* merged, int64_t* snapshot_only, int64_t* gets, int64_t* pairs,
                                int32_t* last_route, double* kernel_ms);
tsq_status tsq_unionstore_cancel(tsq_unionstore* us);
void       tsq_unionstore_destroy(tsq_unionstore* us);

/* ---------------------------------------------------------------- UnionScan: dirty-handle filter + ordered merge
 * Replaces UnionScanExec (executor/union_scan.go:89-300), the operator buildUnionScanFromReader puts above every reader of a table
 * the transaction has written.  Three inputs: the table's DIRTY HANDLES (DirtyTable.addedRows and deletedRows, :56-74; a snapshot row
 * whose handle is in either set is dropped, :212-220), the transaction's own ADDED ROWS in scan order (the mem readers', already
 * filtered by the reader's ranges and conditions — which is why the handles are passed separately: the added set is the table's),
 * and the child's SNAPSHOT rows in scan order.  The output is the row sequence getOneRow produces: the two-way merge of the kept
 * snapshot rows and the added rows under compare (:256-280) — the n_keys index columns with CompareDatum (NULL smaller than every
 * value and equal to NULL; signed / unsigned / real columns as the images of tsq_sort_*, float32 widened, -0.0 == +0.0, NaN
 * greatest; strings byte-wise, the shorter first), then the handle as a SIGNED int64 on its raw 8 bytes whatever the column's type
 * (GetInt64, :269-270); desc inverts the whole tuple, both inputs then arrive descending.  A kept snapshot row and an added row never
 * compare equal.  Both inputs must be sorted in scan order (the reference does not check either): for unsorted input the rows that
 * come out are unspecified, but every index the kernels compute stays in range.
 *
 * STREAMING RULE.  Let S be the kept snapshot rows pushed so far and A the added rows.  Before tsq_unionscan_finish the rows that may
 * be pulled are merge(S, A[0:m)), m = the number of added rows that precede the LAST row of S in scan order (0 while S is empty);
 * after finish, merge(S, A).  So every push is self-contained: its kept rows are merged with the next added rows from a cursor, the
 * result is appended to the output queue, and no snapshot row waits for a later push.  The output sequence does not depend on how
 * the snapshot rows were cut into pushes.  tsq_unionscan_pull answers 0 rows with *eos = 0 when more input is needed; *eos = 1 comes
 * only after finish, once everything has been handed out.  Calls in the wrong order (set_added after a push or twice, push after
 * finish) answer TSQ_ERR_INVALID with a tsq_last_error text; after tsq_unionscan_cancel every call answers TSQ_ERR_CANCELLED.
 *
 * The handle set is an open-addressing table of tsq_unionscan_set_slots(n_added + n_deleted) slots (a power of two, at least twice the
 * handles) with an occupancy bitmap — every int64 is a legal handle; slot of handle h = tsq_mix64-style finaliser of h, masked, then
 * linear probing.  No handles at all: the probe is skipped.  Limits: fewer than 2^31 rows per push and 2^31 added rows. */
typedef struct tsq_unionscan_cfg {
    int32_t n_cols;
    int32_t col_types[TSQ_MAX_COLS];
    int32_t handle_col;                   /* belowHandleIndex; an 8-byte integer column (TSQ_I64 / TSQ_U64), NOT NULL */
    int32_t n_keys;                       /* usedIndex; 0 = a table reader: handle order */
    int32_t key_col[TSQ_MAX_KEYS];        /* most significant first; any column type, strings included */
    int32_t desc;                         /* the reader's desc */
    int32_t max_chunk_size;
} tsq_unionscan_cfg;
typedef struct tsq_unionscan tsq_unionscan;
int64_t    tsq_unionscan_set_slots(int64_t n_handles);
/* added_handles / deleted_handles: host arrays, copied (either may be NULL when its count is 0; duplicates allowed) */
tsq_status tsq_unionscan_create(tsq_ctx* ctx, const tsq_unionscan_cfg* cfg, const int64_t* added_handles, int64_t n_added,
                                const int64_t* deleted_handles, int64_t n_deleted, tsq_unionscan** out);
/* as tsq_unionscan_create, but the two handle arrays are DEVICE memory (what tsq_membuf_dirty_fetch writes) and the set is built by a
 * kernel: same slots, same finaliser, same linear probing.  Every handle, duplicates included, claims the first unoccupied slot on its
 * probe path, so duplicates may lie elsewhere than after the host build; what a probe answers (member / not member) is identical */
tsq_status tsq_unionscan_create_dev(tsq_ctx* ctx, const tsq_unionscan_cfg* cfg, const int64_t* added_handles, int64_t n_added,
                                    const int64_t* deleted_handles, int64_t n_deleted, tsq_unionscan** out);
/* the added rows in scan order: at most once, before the first push; host or TSQ_COL_DEVICE columns, copied */
tsq_status tsq_unionscan_set_added(tsq_unionscan* u, const tsq_col* cols, int32_t n_cols, int64_t nrows);
/* one snapshot chunk in scan order; host or TSQ_COL_DEVICE columns; nothing of the caller is kept after the call */
tsq_status tsq_unionscan_push(tsq_unionscan* u, const tsq_col* cols, int32_t n_cols, int64_t nrows);
tsq_status tsq_unionscan_finish(tsq_unionscan* u);   /* the child is exhausted */
/* as tsq_sort_peek: rows of the next pull of up to cap_rows rows and the data bytes of its var-len columns */
tsq_status tsq_unionscan_peek(tsq_unionscan* u, int64_t cap_rows, int64_t* nrows_out, int64_t* bytes_out, int32_t n_cols);
/* out_cols: the input schema; host or TSQ_COL_DEVICE buffers for cap_rows rows, as tsq_sort_pull */
tsq_status tsq_unionscan_pull(tsq_unionscan* u, tsq_col* out_cols, int32_t n_cols, int64_t cap_rows, int64_t* nrows_out, int32_t* eos);
/* snapshot_rows: pushed; dropped_rows: of those, the ones whose handle was dirty; added_rows_out: added rows emitted so far */
tsq_status tsq_unionscan_stats(tsq_unionscan* u, int64_t* snapshot_rows, int64_t* dropped_rows, int64_t* added_rows_out, double* kernel_ms);
tsq_status tsq_unionscan_cancel(tsq_unionscan* u);
void       tsq_unionscan_destroy(tsq_unionscan* u);

/* ---------------------------------------------------------------- ANALYZE TABLE: column sketches and samples (DESIGN.md "ANALYZE")
 * Replaces SampleBuilder.CollectColumnStats + SampleCollector.collect (statistics/sample.go:206-250, 143-177) as
 * handleCopAnalyzeRequest drives them (store/mockstore/mocktikv/analyze.go:34-219), for up to TSQ_MAX_COLS columns of a scanned chunk.
 * Per non-NULL cell, e = the datum bytes tsq_rows_encode writes for the column type and col_flags (TSQ_ENC_COMPARABLE), or the cell
 * itself for a TSQ_AN_RAW column (TSQ_BYTES; the key prefixes of an index, analyze.go:94-100):
 *   count += 1, total_size += len(e) - 1;
 *   CM sketch (cm_depth x cm_width uint32 counters, at most 16384; both 0 = none): (h1, h2) = murmur3 x64_128 of e, seed 0; for row
 *     i < depth counter (h1 + h2 * i) mod width += 1 (uint64 wrap-around in the index); cm_count += 1;
 *   FM sketch: h1 of the same murmur3 over e — or, with TSQ_AN_WRAP_BYTES, over compactBytesFlag + varint(len e) + e, the bytes datum
 *     the storage side hands FMSketch.InsertValue (analyze.go:236, fmsketch.go:66).  The result is CANONICAL: fm_mask = 2^k - 1 for
 *     the smallest k at which the distinct hashes with h & mask == 0 number at most max_fm_size (>= 1), and the set is those hashes —
 *     independent of row order and push boundaries; equal to the reference's sequential sketch whenever that ends within its limit;
 *   sample: key(r) = splitmix64(sample_seed ^ r), r = the 0-based ordinal of the row among all pushed rows; the sample is the
 *     non-NULL rows with the max_sample_size smallest keys, in row order (all non-NULL rows when there are no more than that).
 * A NULL cell counts in null_count only.  Columns are host or TSQ_COL_DEVICE; any number of pushes, then finish, then the getters. */
#define TSQ_AN_RAW 2u         /* tsq_analyze_cfg.col_flags (beside TSQ_ENC_COMPARABLE) */
#define TSQ_AN_WRAP_BYTES 1u  /* tsq_analyze_cfg.flags */
#define TSQ_AN_MAX_CM_COUNTERS 16384
typedef struct tsq_analyze_cfg {
    int32_t  n_cols;
    int32_t  col_types[TSQ_MAX_COLS];
    uint32_t col_flags[TSQ_MAX_COLS];
    int32_t  reserved;
    int64_t  max_sample_size;   /* colReq.SampleSize */
    int64_t  max_fm_size;       /* colReq.SketchSize */
    int32_t  cm_depth, cm_width;
    uint32_t flags;
    uint32_t reserved2;
    uint64_t sample_seed;
} tsq_analyze_cfg;
typedef struct tsq_analyze tsq_analyze;
tsq_status tsq_analyze_create(tsq_ctx* ctx, const tsq_analyze_cfg* cfg, tsq_analyze** out);
tsq_status tsq_analyze_push(tsq_analyze* a, const tsq_col* cols, int32_t n_cols, int64_t nrows);
tsq_status tsq_analyze_finish(tsq_analyze* a);
/* after finish; any out pointer may be NULL */
tsq_status tsq_analyze_column(tsq_analyze* a, int32_t c, int64_t* null_count, int64_t* count, int64_t* total_size, uint64_t* fm_mask,
                              int64_t* fm_size, int64_t* cm_count, int64_t* n_samples);
tsq_status tsq_analyze_fm(tsq_analyze* a, int32_t c, uint64_t* hashes_out, int64_t cap);     /* fm_size hashes, ascending */
tsq_status tsq_analyze_cm(tsq_analyze* a, int32_t c, uint32_t* counters_out);                /* depth * width, row-major */
/* the sample of column c in row order: out (a HOST column: data, and offsets[cap + 1] for TSQ_BYTES) and the rows' ordinals;
 * tsq_analyze_samples_peek tells the rows and, for a var-len column, the data bytes (as tsq_sort_peek does for a pull) */
tsq_status tsq_analyze_samples_peek(tsq_analyze* a, int32_t c, int64_t* n_samples, int64_t* bytes_out);
tsq_status tsq_analyze_samples(tsq_analyze* a, int32_t c, tsq_col* out, int64_t* ordinals_out, int64_t cap);
tsq_status tsq_analyze_stats(tsq_analyze* a, int64_t* rows, double* kernel_ms);
tsq_status tsq_analyze_cancel(tsq_analyze* a);
void       tsq_analyze_destroy(tsq_analyze* a);

/* ---------------------------------------------------------------- ANALYZE TABLE: the histogram of a sorted stream
 * Replaces SortedBuilder.Iterate (statistics/builder.go:24-94) with Histogram.AppendBucket / updateLastBucket / mergeBuckets
 * (statistics/histogram.go:155-166, 341-358): the PK histogram (sample.go:235-241) and handleAnalyzeIndexReq (analyze.go:79-105).
 * Rows are kept in HBM until finish (col_type TSQ_I64 | TSQ_U64 | TSQ_BYTES; NULL cells are not expected: a bitmap is ignored).  The
 * builder only asks whether a row equals the one before it, so the order of the input is the caller's contract; an unsorted input
 * is no error.  Result: cumulative counts, the repeats of every bucket's upper bound, and the bounds both as row numbers of the input
 * and as values (lower / upper: HOST columns for n_buckets rows; a TSQ_BYTES column with offsets[n_buckets + 1] and the data bytes
 * tsq_sorted_hist_peek tells).  num_buckets = 1 can open more buckets than it names, as in the reference; peek tells how many. */
typedef struct tsq_sorted_hist tsq_sorted_hist;
tsq_status tsq_sorted_hist_create(tsq_ctx* ctx, int32_t col_type, int64_t num_buckets, tsq_sorted_hist** out);
tsq_status tsq_sorted_hist_push(tsq_sorted_hist* h, const tsq_col* col, int64_t nrows);
tsq_status tsq_sorted_hist_finish(tsq_sorted_hist* h);
tsq_status tsq_sorted_hist_peek(tsq_sorted_hist* h, int64_t* n_buckets, int64_t* lower_bytes, int64_t* upper_bytes);
tsq_status tsq_sorted_hist_result(tsq_sorted_hist* h, int64_t* n_buckets, int64_t* count, int64_t* ndv, int64_t* counts, int64_t* repeats,
                                  int64_t* lower_rows, int64_t* upper_rows, tsq_col* lower, tsq_col* upper);
/* scan_ms: run heads + their positions; walk_ms: the one-workgroup bucket walk; steps: absorb searches the walk made */
tsq_status tsq_sorted_hist_stats(tsq_sorted_hist* h, int64_t* rows, double* scan_ms, double* walk_ms, int64_t* steps);
void       tsq_sorted_hist_destroy(tsq_sorted_hist* h);

/* ---------------------------------------------------------------- multi-GPU radix redistribute
 * Splits rows by rank(key) = ((mix64(key) & 0xffff) * n_parts) >> 16 into n_parts contiguous
 * runs (CPU analogue: aggregate.go:352-356 shuffle / join.go:219 dispatch).  The exchange
 * itself (RCCL all-to-all over xGMI) is done by the caller on the returned device buffers.
 * key_mode 0 ranks by join-key equality (util/codec/codec.go:212-240), 1 by group-key equality
 * (codec.go:713-746: -0.0 and +0.0 share a group).  Rows with a NULL key are routed to part 0.
 * cols/out_cols are device resident; out_cols need capacity nrows; counts_out: int64[n_parts]
 * on the host; run p of every output column is rows [sum(counts[0..p)), +counts[p]).
 * Var-len (TSQ_BYTES) columns travel with their rows — as payload, or as the key (equal strings rank alike: a hash of the bytes):
 * their out column needs offsets[nrows + 1] and as many data bytes as the input column holds; the cells are laid out in the order
 * of the split rows. */
tsq_status tsq_radix_split(tsq_ctx* ctx, const tsq_col* cols, int32_t n_cols, int32_t key_col,
                           int32_t key_mode, int64_t nrows, int32_t n_parts, tsq_col* out_cols,
                           int64_t* counts_out);

/* ---------------------------------------------------------------- multi-GPU exchange (RCCL over xGMI), one process per GPU
 * What the reference does with goroutines and channels inside one process — HashJoinExec handing outer chunks to its join
 * workers (executor/join.go:160-231), HashAggExec shuffling partial results to its final workers by group key
 * (executor/aggregate.go:352-356) — across the GPUs of a node: the rank of a key (((mix64(key word) & 0xffff) * world) >> 16, as in tsq_radix_split) owns it.
 * Every rank runs the same call sequence.  Bootstrap: rank 0 calls tsq_comm_unique_id and hands the 128 bytes to the other
 * ranks by any side channel (the Go host: the coordinator's RPC; the harness: a file), then every rank calls tsq_comm_create.
 *
 * tsq_redistribute splits `cols` (device resident; var-len columns included, also as the key) by rank(key) on the
 * context's stream (tsq_radix_split), exchanges the run sizes (rows, and bytes of every var-len column), and queues ONE group of RCCL
 * sends / receives on the communicator's own stream.  A var-len column's run travels as its slice of the offsets plus its bytes; the
 * received column gets offsets[n + 1] rebased onto its own data (out_cols[c].offsets, owned by the slot).  A column with a null bitmap
 * on ANY rank travels with one NOT-NULL byte per row and arrives with a packed bitmap (out_cols[c].null_bitmap, owned by the
 * slot); rows with a NULL key go to rank 0 (they never join; GROUP BY makes them one group).  out_cols describe device
 * buffers owned by `slot` (0..7) of the communicator: they hold the received rows once tsq_redistribute_wait(comm, slot) has
 * made the context's stream wait for the exchange, and stay valid until the next tsq_redistribute on the same slot.  Queue
 * piece c + 1's redistribute before piece c's consumer (wait; tsq_join_probe_push / tsq_agg_push) and the wire time of
 * c + 1 hides behind the operator kernels of c.
 * The all-reduces take up to 8 host words (op 0 sum, 1 max, 2 min) and synchronise both streams: they are the barrier + the
 * COUNT(*) / timing reductions a distributed plan needs. */
#define TSQ_COMM_ID_BYTES 128
tsq_status tsq_comm_unique_id(uint8_t* id_out /* [TSQ_COMM_ID_BYTES] */);
tsq_status tsq_comm_create(tsq_ctx* ctx, int32_t rank, int32_t world, const uint8_t* id, tsq_comm** out);
void       tsq_comm_destroy(tsq_comm* c);
tsq_status tsq_comm_allreduce_i64(tsq_comm* c, int64_t* inout, int32_t n, int32_t op);
tsq_status tsq_comm_allreduce_f64(tsq_comm* c, double* inout, int32_t n, int32_t op);
tsq_status tsq_comm_barrier(tsq_comm* c);
/* ABI 7: the communicator as the collective library sees it — ncclCommUserRank, ncclCommCount, ncclGetVersion (-1: the loaded librccl
 * lacks the call).  bench.py prints them next to a multi-GPU number. */
tsq_status tsq_comm_info(tsq_comm* c, int32_t* rank_out, int32_t* nranks_out, int32_t* rccl_version_out);
/* key_mode of tsq_redistribute: 0 / 1 as for tsq_radix_split; TSQ_KEYMODE_BROADCAST = an ALL-GATHER of the columns — every rank
 * receives every rank's rows, in rank order (key_col is ignored): the small side of a broadcast join (a filtered dimension table,
 * the result of an earlier join) goes to every GPU once, and the big side is never moved (tinysql_amd/parallel.py: dist_q3). */
#define TSQ_KEYMODE_JOIN      0
#define TSQ_KEYMODE_GROUP     1
#define TSQ_KEYMODE_BROADCAST 2
tsq_status tsq_redistribute(tsq_comm* c, const tsq_col* cols, int32_t n_cols, int32_t key_col, int32_t key_mode,
                            int64_t nrows, int32_t slot, tsq_col* out_cols, int64_t* nrows_out);
tsq_status tsq_redistribute_wait(tsq_comm* c, int32_t slot);
/* tsq_redistribute in three calls, for a plan that redistributes its input in PIECES (piece c -> slot c): prepare every piece
 * (the split, on the context's stream), exchange the run sizes of ALL prepared slots with one all-gather (the only call of the
 * three that waits for the other ranks on the host), then issue the pieces one after the other — each issue only queues the
 * sends / receives of its slot behind the previous one.  tsq_redistribute(slot) = prepare(slot) + counts({slot}) + issue(slot).
 * Every rank lists the same slots in the same order. */
tsq_status tsq_redistribute_prepare(tsq_comm* c, const tsq_col* cols, int32_t n_cols, int32_t key_col, int32_t key_mode,
                                    int64_t nrows, int32_t slot);
tsq_status tsq_redistribute_counts(tsq_comm* c, const int32_t* slots, int32_t n_slots);
tsq_status tsq_redistribute_issue(tsq_comm* c, int32_t slot, tsq_col* out_cols, int32_t n_cols, int64_t* nrows_out);

/* ---------------------------------------------------------------- statistics (roofline reporting) */
typedef struct tsq_stats {
    int64_t build_rows;
    int64_t build_rows_inserted;   /* non-NULL keys */
    int64_t probe_rows;
    int64_t out_rows;
    int64_t table_bytes;
    int64_t table_buckets;
    double  build_kernel_ms;       /* HIP-event time of the last build / probe kernels */
    double  probe_kernel_ms;
    int64_t h2d_bytes;
    int64_t d2h_bytes;
    int64_t kernel_launches;
    double  partition_kernel_ms;   /* last radix batch: partition kernel (0 when the direct probe ran) */
    double  radix_probe_kernel_ms; /* last radix batch: partition-at-a-time probe (+ overflow list) kernels */
    double  partition_kernel_ms_sum;    /* HIP-event sums over the most recent radix_timed_batches (<= 32) batches */
    double  radix_probe_kernel_ms_sum;
    int64_t radix_timed_batches;
    int64_t radix_batches;         /* join: probe batches through the radix path; agg: batches pre-aggregated in LDS */
    int64_t radix_overflow_rows;   /* rows that did not fit their partition region (skew) in the last batch */
    int32_t radix_bits;            /* log2(partitions) of the last radix batch */
    int32_t build_partitioned;     /* join: 1: the table was assembled slice by slice in LDS (tsq_buildpart.h), 0: row-at-a-time CAS build;
                                      aggregate: 2: several integer key columns composed into one 64-bit key for a child aggregate, 3: the group
                                      keys (strings / wide key sets) went through the dictionary of key records (tsq_keydict.h) to a child
                                      aggregate by group id; build_handed_back_rows then counts the exception rows this operator kept; 4 (ABI 7): about
                                      as many groups as rows — the group table was a set of partitioned, LDS-sized sub-tables (csrc/tsq_aggfast.h K7p);
                                      when the composite-key child of (2) took that mode, dense_flushes reads -4; 5: a handle of tsq_agg_create_keys with more than
                                      TSQ_MAX_GROUP_KEYS key columns — the keys went through a tsq_groupid to a child aggregate GROUP BY id;
                                      build_handed_back_rows then counts the dictionary's collision rows */
    int64_t build_handed_back_rows; /* partitioned build: rows inserted row by row afterwards (skewed pass-1 / pass-2 regions);
                                       aggregate: rows of a multi-key GROUP BY whose 64-bit tag belonged to another key (resolved) */
    int32_t table_slice_bits;      /* join: log2(slices) of the join table (0: one slice); aggregate on the packed route: bits of a travelling argument cell (16 / 32: narrow cells, 64) */
    int32_t build_slice_retries;   /* 1: a slice overflowed (skewed keys) and the table was rebuilt as one slice */
    int32_t probe_route;           /* route of the last probe batch: TSQ_ROUTE_* */
    int32_t packed_key_bits;       /* TSQ_ROUTE_PACKED: bits of the build side's key range (0 otherwise) */
    double  packed_build_ms;       /* kernels that made the packed-key images (once per build side) */
    int64_t heap_bytes;            /* aggregate: bytes of var-len input cells the operator holds (largest column heap) */
    int64_t heap_compactions;      /* aggregate: times a string heap was compacted to the strings the groups refer to */
    int32_t shared_build;          /* join: 1 = tsq_join_build_finish_shared replicated the packed images (probe rows never cross xGMI) */
    int32_t dense_flushes;         /* aggregate: times the dense partial state of the one-key packed route became groups of the table (1 = at finish only; 0 = route not taken) */
    int64_t shared_image_bytes;    /* ... bytes of the images every rank all-reduced, once per build side */
    double  shared_allreduce_ms;   /* ... wall time of that all-reduce on this rank */
    int64_t div_by_zero_warnings;  /* join: division-by-zero warnings the OtherConditions / outer filters raised so far (NULL result + warning,
                                      expression/errors.go:65-77): the shim appends that many ErrDivisionByZero warnings to the statement context
                                      (handleDivisionByZeroError via executor/joiner.go:155-167) */
    int32_t packed_lds_bits;       /* join, ABI 7: log2 of the FINAL partitions of the last materialising packed batch whose build side sat in LDS
                                      (csrc/tsq_damat.h: two partition levels, ranked payload tables); 0: the batch took another variant */
    int32_t keyrec_digests;        /* join, ABI 7: 1 when the key-record route keeps string cells that do not fit a record as (length, 64-bit digest)
                                      and compares the bytes of every candidate match (long string keys), 0 otherwise */
    int32_t side_stream_batches;   /* aggregate, ABI 7: batches of the packed route whose rows went from the partitioned store into the dense state on the
                                      operator's side stream, beside the partition pass of the next batch (TSQ_KNOB_AGG_OVERLAP) */
    int32_t packed_lds_dup;        /* join, ABI 9 (was reserved0): 1 when the last probe batch took the LDS-build variant for a build side WITH duplicate
                                      keys (csrc/tsq_damat_dup.h; packed_lds_bits is set as on the unique variant), else 0 */
    int64_t str_truncated_warnings; /* join, ABI 8: ErrTruncatedWrongVal / ErrOverflow warnings types.StrToInt appended for the string-valued */
    int64_t str_overflow_warnings;  /* OtherConditions / outer filters so far, one per evaluated row or key-matching pair and kind; a join fails with
                                       the conversion error iff ANY such row or pair raised one */
    int64_t packed_interval_batches; /* join (appended behind the ABI 10 fields): probe batches of the packed COUNT(*) route answered by the range test alone, because
                                       the build side fills its key interval (TSQ_KNOB_DA_INTERVAL, k_da_interval_count); they count in radix_batches too */
} tsq_stats;
#define TSQ_ROUTE_DIRECT     0   /* k_probe_count / k_probe_emit on the table in HBM */
#define TSQ_ROUTE_RADIX_L2   1   /* radix partition, table slices through the XCD's L2 */
#define TSQ_ROUTE_RADIX_LDS  2   /* radix partition, LDS copies of the table slices (64-bit table words) */
#define TSQ_ROUTE_PACKED     3   /* packed keys: 2-byte entries against direct-address images in LDS */
#define TSQ_ROUTE_KEYREC     4   /* key records (ABI 6): several key columns / string keys as 32-byte records, hash-partitioned, matched in LDS (csrc/tsq_keyrec.h) */
tsq_status tsq_join_stats(tsq_join* j, tsq_stats* out);
tsq_status tsq_agg_stats(tsq_agg* a, tsq_stats* out);

#ifdef __cplusplus
}
#endif
#endif /* TSQ_H */
