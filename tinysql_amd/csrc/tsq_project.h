// tsq_project.h — fused Selection + Projection over device chunks (tsq_project_*, ABI 10); included at the end of tsq_expr.hip.
//
// SELECT e1, .., em FROM t WHERE f1 AND .. AND fk is ProjectionExec over SelectionExec in the reference: EvaluatorSuite.Run evaluates the
// whole SELECT list per chunk on the rows the selection kept (expression/evaluator.go:46-63, :121-133, executor/executor.go:393-438).
// As separate operators that is tsq_filter_eval + tsq_chunk_compact (every column copied, read or not) + one tsq_expr_eval per output
// (each a pass over its input columns).  Here:
//   flags     : the filter handle's own path (interpreter or jit_filter), unchanged — expr_run
//   positions : k_compact_count + k_compact_scan (tsq_compact.h): exclusive base of every wave's contiguous run of rows
//   K13       : k_project_eval / jit_project — a wave walks its run in order, ballot + popcount prefix give the dense position, a
//               selected lane evaluates ALL output programs for its row and stores the m results (value + NOT-NULL flag byte, or a
//               string reference) there.  Rows the filter dropped are never evaluated: no error, no division-by-zero count.
//   assembly  : tsq_launch_pack_bitmap per fixed-width output; string references -> k_expr_str_len -> scan -> k_expr_str_copy
// Algorithmic bytes: 8 N per filter column + 1 N flags written + 2 N flags read (count, K13) + 8 B per selected cell of every distinct
// column the outputs read + (8 + 1) m n_out written.  Without filters there are no flags and no positions pass: the row is its position.
// Host round trips for fixed-width outputs: the filter's, the total of the scan (it sizes the outputs), the error word: three.

__device__ __forceinline__ void project_row(const ProjArgs& a, const tsq_expr_prog* progs, int64_t row, int64_t pos, uint64_t& errw, uint32_t& div0) {
    tsq_chunk_src src{&a.in, row};
    for (int j = 0; j < a.n_progs; j++) {
        tsq_val v;
        int node = 0, d0 = 0;
        const tsq_status s = tsq_eval_row(progs[j], src, &v, &node, &d0);
        div0 += (uint32_t)d0;
        if (s != TSQ_OK) {
            const uint64_t w = tsq_errword(j, node, (uint64_t)row, s);
            errw = w < errw ? w : errw;
            continue;
        }
        a.out_data[j][pos] = (uint64_t)v.v;
        a.out_notnull[j][pos] = v.null ? 0 : 1;
    }
}
// K13, interpreter form (the specialised form is jit_project in jit_source)
__global__ void __launch_bounds__(256) k_project_eval(ProjArgs a) {
    __shared__ tsq_expr_prog s_progs[TSQ_EXPR_MAX_PROGS];
    stage_progs(s_progs, a.progs, a.n_progs);
    uint64_t errw = TSQ_ERRWORD_NONE;
    uint32_t div0 = 0;
    if (a.selected == nullptr) {
        const int64_t stride = (int64_t)gridDim.x * blockDim.x;
        for (int64_t i = (int64_t)blockIdx.x * blockDim.x + threadIdx.x; i < a.nrows; i += stride) project_row(a, s_progs, i, i, errw, div0);
    } else {
        const int lane = threadIdx.x & 63;
        const int64_t u = (int64_t)blockIdx.x * 4 + (threadIdx.x >> 6);  // this wave's run of rows
        const int64_t lo = u * a.rows_per_wave;                          // a multiple of 64
        int64_t hi = lo + a.rows_per_wave;
        hi = hi < a.nrows ? hi : a.nrows;
        unsigned long long cur = lo < a.nrows ? a.wave_base[u] : 0ull;  // first output row of the run (wave uniform)
        for (int64_t r = lo + lane; r - lane < hi; r += 64) {
            const bool sel = r < hi && a.selected[r];
            const unsigned long long m = __ballot(sel);
            const unsigned long long pos = cur + __popcll(m & ((1ull << lane) - 1ull));
            cur += (unsigned long long)__popcll(m);
            if (sel) project_row(a, s_progs, r, (int64_t)pos, errw, div0);
        }
    }
    if (errw != TSQ_ERRWORD_NONE) atomicMin(&a.counters[0], (unsigned long long)errw);
    if (div0) atomicAdd(&a.counters[1], (unsigned long long)div0);
}

struct tsq_project {
    tsq_handle_hdr hdr;
    tsq_ctx* ctx = nullptr;
    tsq_expr* filt = nullptr;  // the CNF list (nullptr: a pure projection): its flags, errors and warnings are tsq_filter_eval's
    std::vector<tsq_expr_prog> outs;
    DevBuf progs_d, counters, flags, base, scan_tmp;
    struct Out {
        DevBuf data, nn, bitmap, offs, bytes;  // data: values, or the string references of a string-valued root
    } o[TSQ_EXPR_MAX_PROGS];
    DevEvent ev0, ev1;
    int32_t jit_mode = TSQ_JIT_AUTO;
    bool jit_tried = false;
    std::string jit_src, jit_log;
    hipFunction_t jit_fn = nullptr;
    int64_t rows_seen = 0, launches = 0, jit_launches = 0;
    double eval_ms = 0;
    int64_t str_trunc = 0, str_ovf = 0;
    ~tsq_project() {  // the filter handle first; the buffers and events are released by their own destructors
        if (filt) tsq_expr_destroy(filt);
    }
};

namespace {

// the same gate as jit_launch: false -> the interpreter kernel serves this run
bool project_jit_launch(tsq_project* p, ProjArgs& a, int grid) {
    if (p->jit_mode == TSQ_JIT_OFF) return false;
    if (p->jit_mode == TSQ_JIT_AUTO && p->rows_seen + a.nrows < TSQ_JIT_AUTO_ROWS) return false;
    if (!p->jit_tried) {
        tsq_ctx* ctx = p->ctx;
        if (p->jit_src.empty()) p->jit_src = jit_source(p->outs, (int)tsq_knob(ctx, TSQ_KNOB_JIT_VARIANT, TSQ_JIT_VARIANT_DEFAULT), true);
        tsq_ctx::JitEntry* ent = jit_entry(ctx, p->jit_src, p->jit_mode == TSQ_JIT_FORCE, true);
        if (!ent) return false;
        p->jit_tried = true;
        p->jit_fn = ent->f_project;
        p->jit_log = ent->log;
    }
    if (!p->jit_fn) return false;
    void* params[] = {&a};
    if (hipModuleLaunchKernel(p->jit_fn, (unsigned)grid, 1, 1, 256, 1, 1, 0, p->ctx->stream, params, nullptr) != hipSuccess) {
        (void)hipGetLastError();
        return false;
    }
    p->jit_launches++;
    return true;
}

int32_t project_out_type(const tsq_expr_prog& g) {
    return g.result_type == TSQ_BYTES ? TSQ_BYTES : (g.result_type == TSQ_F64 ? TSQ_F64 : (g.result_unsigned ? TSQ_U64 : TSQ_I64));
}

// out_cols[j] = n rows of output j in the handle's buffers (borrowed by the caller)
void project_fill_out(tsq_project* p, tsq_col* out_cols, int64_t n) {
    for (size_t j = 0; j < p->outs.size(); j++) {
        tsq_col& c = out_cols[j];
        tsq_project::Out& o = p->o[j];
        memset(&c, 0, sizeof c);
        c.type = project_out_type(p->outs[j]);
        const bool str = c.type == TSQ_BYTES;
        c.data = str ? o.bytes.p : o.data.p;
        c.null_bitmap = o.bitmap.as<uint8_t>();
        c.offsets = str ? o.offs.as<int64_t>() : nullptr;
        c.length = n;
        c.elem_size = str ? -1 : 8;
        c.flags = TSQ_COL_DEVICE | TSQ_COL_BORROW;
    }
}

tsq_status project_run(tsq_project* p, const tsq_col* in_cols, int32_t n_cols, int64_t nrows, tsq_col* out_cols, int64_t* nrows_out, int64_t* div0_out) {
    tsq_ctx* ctx = p->ctx;
    tsq_handle_hdr* h = &p->hdr;
    const int m = (int)p->outs.size();
    p->str_trunc = p->str_ovf = 0;
    project_fill_out(p, out_cols, 0);
    if (n_cols < 0 || n_cols > TSQ_MAX_COLS || (n_cols > 0 && !in_cols)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_project_run: bad input columns");
    int32_t ctypes[TSQ_MAX_COLS];
    for (int c = 0; c < n_cols; c++) {
        if (!(in_cols[c].flags & TSQ_COL_DEVICE)) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_project_run: the input columns must be device resident (TSQ_COL_DEVICE)");
        if (in_cols[c].type < TSQ_I64 || in_cols[c].type > TSQ_BYTES) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_project_run: unknown column type");
        if (in_cols[c].length < nrows) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_project_run: column shorter than nrows");
        if (nrows > 0 && (in_cols[c].type == TSQ_BYTES ? !in_cols[c].offsets : !in_cols[c].data))
            return tsq_fail(h, TSQ_ERR_INVALID, "tsq_project_run: column without data (or a var-len column without offsets)");
        ctypes[c] = in_cols[c].type;
    }
    for (int j = 0; j < m; j++) {
        const char* why = "";
        const tsq_status s = tsq_validate_prog(p->outs[j], n_cols, &why, ctypes);
        if (s != TSQ_OK) return tsq_fail(h, s, std::string("tsq_project_run: output ") + std::to_string(j) + ": " + why);
    }
    if (p->filt && n_cols == 0) return tsq_fail(h, TSQ_ERR_INVALID, "tsq_project_run: a filter needs at least one (device-resident) input column");
    if (nrows == 0) return TSQ_OK;
    TSQ_HIP(h, hipSetDevice(ctx->device));

    // ---- flags: exactly tsq_filter_eval (its errors come first and end the run; its warnings are this run's)
    int64_t div0 = 0;
    ProjArgs a;
    memset(&a, 0, sizeof a);
    tsq_colset_from_cols(a.in, in_cols, n_cols);
    a.progs = p->progs_d.as<tsq_expr_prog>();
    a.n_progs = m;
    a.nrows = nrows;
    a.counters = p->counters.as<unsigned long long>();
    int64_t n_out = nrows;
    const int grid = tsq_grid_for(ctx, nrows, 256);
    if (p->filt) {
        TSQ_TRY(p->flags.reserve(ctx, h, (size_t)nrows + 64));
        p->filt->jit_mode = p->jit_mode;
        const tsq_status fs = expr_run(p->filt, true, in_cols, n_cols, nrows, nullptr, nullptr, p->flags.as<uint8_t>(), nullptr, &div0);
        p->str_trunc = p->filt->str_trunc;
        p->str_ovf = p->filt->str_ovf;
        if (div0_out) *div0_out = div0;
        if (fs != TSQ_OK) return tsq_fail(h, fs, "tsq_project_run: filter: " + p->filt->hdr.err);
        // ---- positions: per-wave counts -> exclusive bases; the total sizes the outputs
        const int n_runs = grid * 4;
        CompactArgs ca;
        memset(&ca, 0, sizeof ca);
        ca.selected = p->flags.as<uint8_t>();
        ca.nrows = nrows;
        ca.rows_per_wave = (((nrows + n_runs - 1) / n_runs) + 63) & ~(int64_t)63;
        TSQ_TRY(p->base.reserve(ctx, h, (size_t)n_runs * 8 + 64));
        ca.block_base = p->base.as<unsigned long long>();
        ca.total = ca.block_base + n_runs;
        hipLaunchKernelGGL(k_compact_count, dim3(grid), dim3(256), 0, ctx->stream, ca);
        hipLaunchKernelGGL(k_compact_scan, dim3(1), dim3(1024), 0, ctx->stream, ca.block_base, n_runs, ca.total);
        TSQ_HIP(h, hipGetLastError());
        TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 16, ca.total, 8, hipMemcpyDeviceToHost, ctx->stream));
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
        n_out = (int64_t)ctx->pinned[16];
        if (n_out < 0 || n_out > nrows) return tsq_fail(h, TSQ_ERR_HIP, "tsq_project_run: the positions pass counted more rows than the chunk has");
        a.selected = ca.selected;
        a.rows_per_wave = ca.rows_per_wave;
        a.wave_base = ca.block_base;
    }
    if (n_out == 0) return TSQ_OK;

    // ---- K13: all outputs of every selected row, at its dense position
    for (int j = 0; j < m; j++) {
        TSQ_TRY(p->o[j].data.reserve(ctx, h, (size_t)n_out * 8 + 64));
        TSQ_TRY(p->o[j].nn.reserve(ctx, h, (size_t)n_out + 64));
        TSQ_TRY(p->o[j].bitmap.reserve(ctx, h, tsq_bitmap_bytes(n_out) + 64));
        a.out_data[j] = p->o[j].data.as<uint64_t>();
        a.out_notnull[j] = p->o[j].nn.as<uint8_t>();
    }
    TSQ_HIP(h, hipMemsetAsync(a.counters, 0xff, 8, ctx->stream));
    TSQ_HIP(h, hipMemsetAsync(a.counters + 1, 0, 8, ctx->stream));
    TSQ_HIP(h, hipEventRecord(p->ev0, ctx->stream));
    if (!project_jit_launch(p, a, grid)) hipLaunchKernelGGL(k_project_eval, dim3(grid), dim3(256), 0, ctx->stream, a);
    TSQ_HIP(h, hipGetLastError());
    TSQ_HIP(h, hipEventRecord(p->ev1, ctx->stream));
    p->launches++;
    p->rows_seen += nrows;
    bool any_str = false;
    for (int j = 0; j < m; j++) {
        any_str = any_str || p->outs[j].result_type == TSQ_BYTES;
        TSQ_TRY(tsq_launch_pack_bitmap(ctx, h, a.out_notnull[j], p->o[j].bitmap.as<uint8_t>(), n_out));
    }
    TSQ_HIP(h, hipMemcpyAsync(ctx->pinned, a.counters, 16, hipMemcpyDeviceToHost, ctx->stream));
    TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    float ms = 0;
    if (hipEventElapsedTime(&ms, p->ev0, p->ev1) == hipSuccess) p->eval_ms = ms;
    else (void)hipGetLastError();
    div0 += (int64_t)ctx->pinned[1];
    if (div0_out) *div0_out = div0;
    TSQ_TRY(errword_status(h, ctx->pinned[0], "output"));

    // ---- string-valued outputs: references at dense positions -> lengths -> offsets -> bytes (the K9s chain of tsq_expr_eval_str)
    if (any_str) {
        const int sgrid = tsq_grid_for(ctx, n_out, 256);
        for (int j = 0; j < m; j++) {
            if (p->outs[j].result_type != TSQ_BYTES) continue;
            StrRootArgs sa;
            memset(&sa, 0, sizeof sa);
            sa.refs = a.out_data[j];
            sa.notnull = a.out_notnull[j];
            sa.nrows = n_out;
            sa.in = a.in;
            sa.prog = a.progs + j;
            TSQ_TRY(p->o[j].offs.reserve(ctx, h, ((size_t)n_out + 2) * 8));
            sa.offs = p->o[j].offs.as<int64_t>();
            hipLaunchKernelGGL(k_expr_str_len, dim3(sgrid), dim3(256), 0, ctx->stream, sa);
            TSQ_HIP(h, hipGetLastError());
            TSQ_TRY(tsq_launch_scan64(ctx, h, sa.offs, n_out, p->scan_tmp));
            TSQ_HIP(h, hipMemcpyAsync(ctx->pinned + 2, sa.offs + n_out, 8, hipMemcpyDeviceToHost, ctx->stream));
            TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
            const int64_t nbytes = (int64_t)ctx->pinned[2];
            TSQ_TRY(p->o[j].bytes.reserve(ctx, h, (size_t)nbytes + 64));
            sa.data = p->o[j].bytes.as<uint8_t>();
            if (nbytes > 0) {
                if (nbytes / n_out > 32) hipLaunchKernelGGL(k_expr_str_copy<true>, dim3(ctx->num_cus * 8), dim3(256), 0, ctx->stream, sa);
                else hipLaunchKernelGGL(k_expr_str_copy<false>, dim3(sgrid), dim3(256), 0, ctx->stream, sa);
                TSQ_HIP(h, hipGetLastError());
            }
        }
        TSQ_HIP(h, hipStreamSynchronize(ctx->stream));
    }
    project_fill_out(p, out_cols, n_out);
    *nrows_out = n_out;
    return TSQ_OK;
}

}  // namespace

TSQ_API tsq_status tsq_project_create(tsq_ctx* ctx, const tsq_expr_prog* filters, int32_t n_filters, const tsq_expr_prog* outputs, int32_t n_outputs,
                                      tsq_project** out) {
    tsq_ctx_lock _api_lock(ctx);
    if (!ctx || ctx->hdr.magic != TSQ_MAGIC_CTX || !out) return tsq_fail(ctx && ctx->hdr.magic == TSQ_MAGIC_CTX ? &ctx->hdr : nullptr, TSQ_ERR_INVALID, "tsq_project_create: bad arguments");
    *out = nullptr;
    tsq_handle_hdr* ch = &ctx->hdr;
    if (n_outputs < 1 || n_outputs > TSQ_EXPR_MAX_PROGS || !outputs) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_project_create: n_outputs must be 1..16");
    if (n_filters < 0 || n_filters > TSQ_EXPR_MAX_PROGS || (n_filters > 0 && !filters)) return tsq_fail(ch, TSQ_ERR_INVALID, "tsq_project_create: n_filters must be 0..16");
    for (int j = 0; j < n_outputs; j++) {
        const char* why = "";
        const tsq_status s = tsq_validate_prog(outputs[j], -1, &why);
        if (s != TSQ_OK) return tsq_fail(ch, s, std::string("tsq_project_create: output ") + std::to_string(j) + ": " + why);
    }
    TSQ_HIP(ch, hipSetDevice(ctx->device));
    std::unique_ptr<tsq_project> p(new tsq_project());
    p->hdr.magic = TSQ_MAGIC_PROJECT;
    p->ctx = ctx;
    p->outs.assign(outputs, outputs + n_outputs);
    tsq_status s = TSQ_OK;
    if (n_filters > 0) s = tsq_expr_compile(ctx, filters, n_filters, &p->filt);  // (validates the conjuncts; its message is the context's)
    if (s == TSQ_OK) s = p->progs_d.reserve(ctx, &p->hdr, sizeof(tsq_expr_prog) * n_outputs);
    if (s == TSQ_OK) s = p->counters.reserve(ctx, &p->hdr, 64);
    if (s == TSQ_OK) {
        hipError_t err = hipMemcpy(p->progs_d.p, outputs, sizeof(tsq_expr_prog) * n_outputs, hipMemcpyHostToDevice);
        if (err == hipSuccess) err = p->ev0.create();
        if (err == hipSuccess) err = p->ev1.create();
        if (err != hipSuccess) s = tsq_fail(&p->hdr, TSQ_ERR_HIP, hipGetErrorString(err));
    }
    if (s != TSQ_OK) {
        if (!p->hdr.err.empty()) tsq_fail(ch, s, p->hdr.err);
        (void)hipStreamSynchronize(ctx->stream);  // before the handle's buffers go
        return s;
    }
    *out = p.release();
    return TSQ_OK;
}

TSQ_API tsq_status tsq_project_run(tsq_project* p, const tsq_col* in_cols, int32_t n_cols, int64_t nrows, tsq_col* out_cols, int32_t n_out_cols,
                                   int64_t* nrows_out, int64_t* div_by_zero_warnings) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(p, TSQ_MAGIC_PROJECT));
    if (!p || p->hdr.magic != TSQ_MAGIC_PROJECT) return TSQ_ERR_INVALID;
    if (!out_cols || !nrows_out || nrows < 0 || n_out_cols != (int32_t)p->outs.size())
        return tsq_fail(&p->hdr, TSQ_ERR_INVALID, "tsq_project_run: out_cols / nrows_out == NULL, nrows < 0 or n_out_cols != the number of outputs");
    *nrows_out = 0;
    if (div_by_zero_warnings) *div_by_zero_warnings = 0;
    return project_run(p, in_cols, n_cols, nrows, out_cols, nrows_out, div_by_zero_warnings);
}

TSQ_API tsq_status tsq_project_set_jit(tsq_project* p, int32_t mode) {
    if (!p || p->hdr.magic != TSQ_MAGIC_PROJECT) return TSQ_ERR_INVALID;
    if (mode < TSQ_JIT_AUTO || mode > TSQ_JIT_FORCE) return tsq_fail(&p->hdr, TSQ_ERR_INVALID, "mode must be -1 (auto), 0 (off) or 1 (force)");
    p->jit_mode = mode;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_project_str_warnings(tsq_project* p, int64_t* truncated, int64_t* overflow) {
    if (!p || p->hdr.magic != TSQ_MAGIC_PROJECT) return TSQ_ERR_INVALID;
    if (truncated) *truncated = p->str_trunc;
    if (overflow) *overflow = p->str_ovf;
    return TSQ_OK;
}

TSQ_API tsq_status tsq_project_stats(tsq_project* p, int64_t* eval_launches, int64_t* jit_launches, double* eval_kernel_ms) {
    if (!p || p->hdr.magic != TSQ_MAGIC_PROJECT) return TSQ_ERR_INVALID;
    if (p->jit_tried && !p->jit_fn) tsq_fail(&p->hdr, TSQ_OK, std::string("expression JIT unavailable: ") + p->jit_log.substr(0, 600));
    if (eval_launches) *eval_launches = p->launches;
    if (jit_launches) *jit_launches = p->jit_launches;
    if (eval_kernel_ms) *eval_kernel_ms = p->eval_ms;
    return TSQ_OK;
}

TSQ_API void tsq_project_destroy(tsq_project* p) {
    tsq_ctx_lock _api_lock(tsq_ctx_of(p, TSQ_MAGIC_PROJECT));
    if (!p || p->hdr.magic != TSQ_MAGIC_PROJECT) return;
    (void)hipSetDevice(p->ctx->device);
    (void)hipStreamSynchronize(p->ctx->stream);
    // (the specialised module stays in the context's plan cache, as for tsq_expr)
    p->hdr.magic = 0;
    delete p;
}
