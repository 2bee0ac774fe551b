// lp_batch_host.inc -- host side of a batch of independent LPs: the argument checks, the buffers of a solve, its passes
// (wg_queue_host.inc) and what the C ABI reads afterwards.  Included inside the anonymous namespace of lp_batch.hip
// (libyalps_lpbatch.so), milp_batch.hip (libyalps_milpbatch.so, whose root pass is this code with kept tableaux) and lp_sens.hip
// (libyalps_lpsens.so) after wg_queue_host.inc.  A library names itself with a struct X:
//   X::Launch    LpLaunch, or SensLaunch with the buffer of the ranges (X::sens)
//   X::kernels() its KernelTable<X::Launch>
//   X::name      "yalps_lpbatch", in messages;  X::env  "YALPS_LPBATCH", prefix of the environment switches
// and its handle is a struct of the C type's name that derives from LpPass<X>.
template <class X>
struct LpPass : QueueDevice {
    using Lib = X;
    QueueBufs q;
    DevBuf desc, row, col, val;
    // the last solve
    std::vector<LpDesc> descs;
    std::vector<double> h_col0;
    std::vector<int32_t> h_pos, h_var;
    std::string info;
    DevBuf sens;                 // X::sens: per LP 3 * (w + h) doubles at 3 * perm_off: row0[w] col_up[w] col_dn[w] row_lo[h] row_hi[h]
    std::vector<double> h_sens;
};

template <class X>
int lp_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *off, const int32_t *row, const int32_t *col) {
    const std::string name = X::name;
    if (count < 0) return fail(YALPS_E_ARG, name + ": count < 0");
    if (count == 0) return 0;
    if (!width || !height || !off) return fail(YALPS_E_ARG, name + ": width / height / cell_offsets is NULL");
    if (off[0] < 0) return fail(YALPS_E_ARG, name + ": LP 0: negative cell offset");
    for (int32_t i = 0; i < count; i++) {
        const std::string who = name + ": LP " + std::to_string(i) + ": ";
        const int64_t w = width[i], h = height[i];
        if (w < 1 || h < 1) return fail(YALPS_E_ARG, who + "width and height must be at least 1");
        if (8 * w * h > QUEUE_MAX_BYTES)
            return fail(YALPS_E_ARG, who + "tableau of " + std::to_string(8 * w * h) + " bytes is above the batch limit of " +
                                         std::to_string(QUEUE_MAX_BYTES));
        if (off[i + 1] < off[i]) return fail(YALPS_E_ARG, who + "cell offsets decrease");
        if (off[i + 1] > off[i] && (!row || !col)) return fail(YALPS_E_ARG, who + "row / col is NULL");
        int64_t at = 0;
        if (int bad = check_cells(row, col, off[i], off[i + 1], w, h, &at))
            return fail(YALPS_E_ARG, bad == 1 ? who + "cell " + std::to_string(at) + " lies outside the tableau"
                                              : who + "cells are not sorted by (row, col), strictly increasing");
    }
    return 0;
}

template <class H>
void lp_destroy(H *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    release(b->q);
    release({&b->desc, &b->row, &b->col, &b->val, &b->sens});
    close_device(*b);
    delete b;
}

template <class H>
int lp_create_impl(int32_t device, void *hip_stream, H **out) {
    using X = typename H::Lib;
    const std::string env = X::env;
    H *b = new H();
    *out = b;
    if (int rc = open_device(*b, device, hip_stream)) return rc;
    b->q.hist_first = std::max(1, env_int((env + "_HIST").c_str(), (int)HIST_FIRST)); // (test hook: forces the rerun)
    env_list((env + "_LANES").c_str(), b->lanes, HBM_CLASS);
    env_list((env + "_PER_CU").c_str(), b->per_cu, NCLASS);
    for (int k = 0; k < NCLASS; k++) {
        if (!find_form(X::kernels(), b->lanes[k], false, k != HBM_CLASS))
            return fail(YALPS_E_ARG, env + "_LANES: class " + std::to_string(k) + " has no kernel of " + std::to_string(b->lanes[k]) + " lanes (256 or 1024)");
        if (b->per_cu[k] < 1 || b->per_cu[k] > 8) // (32 waves per CU: at most eight workgroups of 256 lanes)
            return fail(YALPS_E_ARG, env + "_PER_CU: class " + std::to_string(k) + ": " + std::to_string(b->per_cu[k]) + " is outside 1..8");
    }
    return raise_lds_limit(X::kernels());
}

// lp_create_impl, with a half-made handle taken down again and the reason kept
template <class H>
int lp_create(int32_t device, void *hip_stream, H **out) {
    *out = nullptr;
    const int rc = lp_create_impl(device, hip_stream, out);
    if (rc && *out) {
        const std::string why = g_err;
        lp_destroy(*out);
        *out = nullptr;
        g_err = why;
    }
    return rc;
}

template <class X>
int lp_solve_impl(LpPass<X> *b, int32_t count, const int32_t *width, const int32_t *height, const int64_t *off, const int32_t *row,
                  const int32_t *col, const double *val, const double *precision, const double *maxPivots, const int32_t *checkCycles,
                  int32_t keep, int32_t *status_out, double *result_out, int64_t *pivots_out, float *gpu_ms_out) {
    const std::string name = X::name;
    if (int rc = lp_validate<X>(count, width, height, off, row, col)) return rc;
    if (count > 0 && (!precision || !maxPivots || !checkCycles || (off[count] > off[0] && !val)))
        return fail(YALPS_E_ARG, name + "_solve: val / precision / maxPivots / checkCycles is NULL");
    b->descs.clear();
    b->q.keep = keep != 0;
    b->info = "launches=0 reruns=0\n";
    if (gpu_ms_out) *gpu_ms_out = 0.f;
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const size_t n = (size_t)count;
    std::vector<LpDesc> &D = b->descs;
    D.resize(n);
    long long col0_total = 0, perm_total = 0, tab_total = 0;
    const int64_t base = off[0];
    for (size_t i = 0; i < n; i++) {
        LpDesc &d = D[i];
        d.w = width[i];
        d.h = height[i];
        d.cell_lo = off[i] - base;
        d.cell_hi = off[i + 1] - base;
        d.col0_off = col0_total;
        d.perm_off = perm_total;
        d.tab_off = tab_total;
        d.precision = precision[i];
        d.max_pivots = maxPivots[i];
        d.aux_hbm = lp_aux_hbm(d.w, d.h) ? 1 : 0;
        d.pad_ = 0;
        col0_total += (d.h + 1) & ~1; // (even offsets: 16-byte aligned column 0)
        perm_total += d.w + d.h;
        tab_total += (long long)d.w * d.h;
    }
    const size_t ncells = (size_t)(off[count] - base);
    if (int rc = ensure(b->desc, sizeof(LpDesc) * n)) return rc;
    if (int rc = ensure(b->row, sizeof(int32_t) * ncells)) return rc;
    if (int rc = ensure(b->col, sizeof(int32_t) * ncells)) return rc;
    if (int rc = ensure(b->val, sizeof(double) * ncells)) return rc;
    if (int rc = ensure_outputs(b->q, n, (size_t)col0_total, (size_t)perm_total, (size_t)tab_total)) return rc;
    if (X::sens)
        if (int rc = ensure(b->sens, sizeof(double) * 3 * (size_t)perm_total)) return rc;
    HIP_TRY(hipMemcpyAsync(b->desc.p, D.data(), sizeof(LpDesc) * n, hipMemcpyHostToDevice, s));
    if (ncells) {
        HIP_TRY(hipMemcpyAsync(b->row.p, row + base, sizeof(int32_t) * ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->col.p, col + base, sizeof(int32_t) * ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->val.p, val + base, sizeof(double) * ncells, hipMemcpyHostToDevice, s));
    }
    if (int rc = reset_status(b->q, s, n)) return rc;

    std::string text;
    QueueRun run;
    const std::string call = name + "_solve";
    const int rc = run_queue(
        *b, b->q, X::kernels(), QueueText{X::name, false, call.c_str(), "LP"}, n,
        [&](int32_t i, int *w, int *h) { return *w = D[i].w, *h = D[i].h, checkCycles[i] != 0; },
        [&](typename X::Launch &a) {
            a.desc = b->desc.template as<const LpDesc>();
            a.row = b->row.template as<const int32_t>();
            a.col = b->col.template as<const int32_t>();
            a.val = b->val.template as<const double>();
            if constexpr (X::sens) a.sens = b->sens.template as<double>();
        },
        [] { return 0; },
        [&](const Launch &L, const std::string &kernel, int pass, int launch, long long hist_cap) {
            char line[256];
            std::snprintf(line, sizeof line, "launch=%d pass=%d kernel=%s class=%d lps=%zu grid=%d lds=%zu hist_cap=%lld\n", launch, pass,
                          kernel.c_str(), L.cls, L.items.size(), L.grid, L.shmem, hist_cap);
            text += line;
        },
        run);
    if (rc) return rc;
    b->info = "launches=" + std::to_string(run.launches) + " reruns=" + std::to_string(run.reruns.size()) + " rerun_lps=[" +
              join_ids(run.reruns) + "]\n" + text;

    b->h_col0.resize((size_t)col0_total);
    b->h_pos.resize((size_t)perm_total);
    b->h_var.resize((size_t)perm_total);
    HIP_TRY(hipMemcpyAsync(b->h_col0.data(), b->q.col0.p, sizeof(double) * (size_t)col0_total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_pos.data(), b->q.pos.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_var.data(), b->q.var.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
    if (X::sens) {
        b->h_sens.resize(3 * (size_t)perm_total);
        HIP_TRY(hipMemcpyAsync(b->h_sens.data(), b->sens.p, sizeof(double) * 3 * (size_t)perm_total, hipMemcpyDeviceToHost, s));
    }
    if (result_out) HIP_TRY(hipMemcpyAsync(result_out, b->q.result.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (pivots_out) HIP_TRY(hipMemcpyAsync(pivots_out, b->q.pivots.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (status_out) std::memcpy(status_out, b->q.h_status.data(), sizeof(int32_t) * n);
    if (gpu_ms_out) *gpu_ms_out = run.ms;
    return 0;
}

// ---- what the C ABI of libyalps_lpbatch.so and libyalps_lpsens.so reads of the last solve; `fn` names the entry in messages ----
template <class X>
int lp_solve(LpPass<X> *b, const char *fn, int32_t count, const int32_t *width, const int32_t *height, const int64_t *off,
             const int32_t *row, const int32_t *col, const double *val, const double *precision, const double *maxPivots,
             const int32_t *checkCycles, int32_t keep, int32_t *status_out, double *result_out, int64_t *pivots_out, float *gpu_ms_out) {
    if (!b) return fail(YALPS_E_ARG, std::string(fn) + ": handle is NULL");
    const int32_t rc = lp_solve_impl(b, count, width, height, off, row, col, val, precision, maxPivots, checkCycles, keep, status_out,
                                     result_out, pivots_out, gpu_ms_out);
    if (rc) b->descs.clear(); // (no last solve to read from)
    return rc;
}

template <class X>
int lp_solution(LpPass<X> *b, const char *fn, int32_t i, double *col0, int32_t *positionOfVariable, int32_t *variableAtPosition) {
    if (!b || i < 0 || (size_t)i >= b->descs.size()) return fail(YALPS_E_ARG, std::string(fn) + ": no such LP in the last solve");
    const LpDesc &d = b->descs[(size_t)i];
    const size_t np = (size_t)d.w + (size_t)d.h;
    if (col0) std::memcpy(col0, b->h_col0.data() + d.col0_off, sizeof(double) * (size_t)d.h);
    if (positionOfVariable) std::memcpy(positionOfVariable, b->h_pos.data() + d.perm_off, sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, b->h_var.data() + d.perm_off, sizeof(int32_t) * np);
    return 0;
}

template <class X>
int lp_tableau(LpPass<X> *b, const char *fn, int32_t i, double *matrix) {
    if (!b || i < 0 || (size_t)i >= b->descs.size() || !matrix) return fail(YALPS_E_ARG, std::string(fn) + ": no such LP in the last solve");
    if (!b->q.keep) return fail(YALPS_E_ARG, std::string(fn) + ": the last solve did not keep its tableaux (keep_tableaux)");
    const LpDesc &d = b->descs[(size_t)i];
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(matrix, b->q.tab.template as<const double>() + d.tab_off, sizeof(double) * (size_t)d.w * (size_t)d.h,
                           hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}
