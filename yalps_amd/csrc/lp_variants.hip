// lp_variants.hip -- libyalps_lpvar.so: many variants of one LP in one call (include/yalps_lpvar.h)
// C ABI, host side and the lp_variants_kernel instantiations.  A library of its own: nothing here is linked into the other
// four, and the pivot loop is libyalps_hip.so's wg_simplex.cuh, included unchanged.  Size classes, the pass and the rerun
// protocol are wg_queue_host.inc, with this library's kernel table; one shape per call means one class, one image and at
// most two launches per pass.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/yalps_lpvar.h"

#pragma clang fp contract(off)

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_variants_kernel.cuh"
#include "wg_queue_host.inc"

static_assert(YALPS_LPVAR_MAX_BYTES == QUEUE_MAX_BYTES, "include/yalps_lpvar.h");
const KernelTable<VarLaunch> kVarKernels = QUEUE_KERNEL_TABLE(lp_variants_kernel);
} // namespace

struct yalps_lpvar : QueueDevice {
    hipEvent_t evb0 = nullptr, evb1 = nullptr; // the image's assembly
    QueueBufs q;
    DevBuf desc, brow, bcol, bval, image, prow, pcol, pval;
    // the last solve
    int32_t w = 0, h = 0, count = 0;
    std::vector<double> h_col0;
    std::vector<int32_t> h_pos, h_var;
    std::string info;
};

namespace {
int validate(int64_t w, int64_t h, int64_t ncells, const int32_t *brow, const int32_t *bcol, int32_t count, const int64_t *off,
             const int32_t *prow, const int32_t *pcol) {
    if (w < 1 || h < 1) return fail(YALPS_E_ARG, "yalps_lpvar: width and height must be at least 1");
    if (8 * w * h > YALPS_LPVAR_MAX_BYTES)
        return fail(YALPS_E_ARG, "yalps_lpvar: tableau of " + std::to_string(8 * w * h) + " bytes is above the limit of " +
                                     std::to_string((long long)YALPS_LPVAR_MAX_BYTES));
    if (ncells < 0) return fail(YALPS_E_ARG, "yalps_lpvar: base_cells < 0");
    if (ncells > 0 && (!brow || !bcol)) return fail(YALPS_E_ARG, "yalps_lpvar: base_row / base_col is NULL");
    int64_t at = 0;
    if (int bad = check_cells(brow, bcol, 0, ncells, w, h, &at))
        return fail(YALPS_E_ARG, bad == 1 ? "yalps_lpvar: base cell " + std::to_string(at) + " lies outside the tableau"
                                          : "yalps_lpvar: base cells are not sorted by (row, col), strictly increasing");
    if (count < 0) return fail(YALPS_E_ARG, "yalps_lpvar: count < 0");
    if (count == 0) return 0;
    if (!off) return fail(YALPS_E_ARG, "yalps_lpvar: patch_offsets is NULL");
    if (off[0] < 0) return fail(YALPS_E_ARG, "yalps_lpvar: variant 0: negative patch offset");
    for (int32_t i = 0; i < count; i++) {
        const std::string who = "yalps_lpvar: variant " + std::to_string(i) + ": ";
        if (off[i + 1] < off[i]) return fail(YALPS_E_ARG, who + "patch offsets decrease");
        if (off[i + 1] > off[i] && (!prow || !pcol)) return fail(YALPS_E_ARG, who + "patch_row / patch_col is NULL");
        if (int bad = check_cells(prow, pcol, off[i], off[i + 1], w, h, &at))
            return fail(YALPS_E_ARG, bad == 1 ? who + "patch cell " + std::to_string(at) + " lies outside the tableau"
                                              : who + "patch cells are not sorted by (row, col), strictly increasing");
    }
    return 0;
}

int create_impl(int32_t device, void *hip_stream, yalps_lpvar **out) {
    yalps_lpvar *b = new yalps_lpvar();
    *out = b;
    if (int rc = open_device(*b, device, hip_stream)) return rc;
    HIP_TRY(hipEventCreate(&b->evb0));
    HIP_TRY(hipEventCreate(&b->evb1));
    b->q.hist_first = std::max(1, env_int("YALPS_LPVAR_HIST", (int)HIST_FIRST)); // (test hook: forces the rerun)
    const int per_cu = env_int("YALPS_LPVAR_PER_CU", 0);                          // (test hook: one value for every class, a small grid)
    if (per_cu < 0 || per_cu > 8) return fail(YALPS_E_ARG, "YALPS_LPVAR_PER_CU: " + std::to_string(per_cu) + " is outside 1..8");
    for (int k = 0; k < NCLASS; k++) b->per_cu[k] = per_cu ? std::min(per_cu, kClasses[k].per_cu) : kClasses[k].per_cu;
    return raise_lds_limit(kVarKernels);
}

int solve_impl(yalps_lpvar *b, int32_t w, int32_t h, int64_t ncells, const int32_t *brow, const int32_t *bcol, const double *bval,
               int32_t count, const int64_t *off, const int32_t *prow, const int32_t *pcol, const double *pval,
               const double *precision, const double *maxPivots, const int32_t *checkCycles, int32_t keep, int32_t *status_out,
               double *result_out, int64_t *pivots_out, float *gpu_ms_out) {
    if (int rc = validate(w, h, ncells, brow, bcol, count, off, prow, pcol)) return rc;
    if (ncells > 0 && !bval) return fail(YALPS_E_ARG, "yalps_lpvar_solve: base_val is NULL");
    if (count > 0 && (!precision || !maxPivots || !checkCycles || (off[count] > off[0] && !pval)))
        return fail(YALPS_E_ARG, "yalps_lpvar_solve: patch_val / precision / maxPivots / checkCycles is NULL");
    b->count = 0;
    b->q.keep = keep != 0;
    b->info = "launches=0 reruns=0\n";
    if (gpu_ms_out) *gpu_ms_out = 0.f;
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(b->device));
    hipStream_t s = b->stream;
    const size_t n = (size_t)count, heven = ((size_t)h + 1) & ~(size_t)1, perm = (size_t)w + (size_t)h;
    // what the call's one shape fixes: its class, whether colbuf / prow go to HBM, and the image in the form's layout
    const int cls = lp_class(w, h);
    const bool lds = cls != HBM_CLASS, aux = !lds && lp_aux_hbm(w, h);
    const int pitch = lds ? small_lds_pitch(w - 1) : small_pcols(w - 1);
    const size_t image_doubles = (size_t)h * pitch + heven;
    const int64_t base = off[0];
    const size_t npatch = (size_t)(off[count] - base);
    std::vector<VarDesc> D(n);
    for (size_t i = 0; i < n; i++) D[i] = VarDesc{off[i] - base, off[i + 1] - base, precision[i], maxPivots[i]};
    if (int rc = ensure(b->desc, sizeof(VarDesc) * n)) return rc;
    if (int rc = ensure(b->brow, sizeof(int32_t) * (size_t)ncells)) return rc;
    if (int rc = ensure(b->bcol, sizeof(int32_t) * (size_t)ncells)) return rc;
    if (int rc = ensure(b->bval, sizeof(double) * (size_t)ncells)) return rc;
    if (int rc = ensure(b->image, sizeof(double) * image_doubles)) return rc;
    if (int rc = ensure(b->prow, sizeof(int32_t) * npatch)) return rc;
    if (int rc = ensure(b->pcol, sizeof(int32_t) * npatch)) return rc;
    if (int rc = ensure(b->pval, sizeof(double) * npatch)) return rc;
    if (int rc = ensure_outputs(b->q, n, heven * n, perm * n, (size_t)w * (size_t)h * n)) return rc;
    HIP_TRY(hipMemcpyAsync(b->desc.p, D.data(), sizeof(VarDesc) * n, hipMemcpyHostToDevice, s));
    if (ncells) {
        HIP_TRY(hipMemcpyAsync(b->brow.p, brow, sizeof(int32_t) * (size_t)ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->bcol.p, bcol, sizeof(int32_t) * (size_t)ncells, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->bval.p, bval, sizeof(double) * (size_t)ncells, hipMemcpyHostToDevice, s));
    }
    if (npatch) {
        HIP_TRY(hipMemcpyAsync(b->prow.p, prow + base, sizeof(int32_t) * npatch, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->pcol.p, pcol + base, sizeof(int32_t) * npatch, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->pval.p, pval + base, sizeof(double) * npatch, hipMemcpyHostToDevice, s));
    }
    if (int rc = reset_status(b->q, s, n)) return rc;
    b->w = w;
    b->h = h;
    b->count = count;

    // the image, once per call: zeros, then the base cells; the solving launches follow on the same stream
    {
        const size_t units = image_doubles / 2;
        const int zgrid = (int)std::min<size_t>((units + 255) / 256, (size_t)b->num_cus * 8);
        const int sgrid = (int)std::min<size_t>(((size_t)ncells + 255) / 256, (size_t)b->num_cus * 8);
        double *image = b->image.as<double>();
        const int32_t *dr = b->brow.as<const int32_t>(), *dc = b->bcol.as<const int32_t>();
        const double *dv = b->bval.as<const double>();
        HIP_TRY(hipEventRecord(b->evb0, s));
        lp_variants_base_kernel<<<dim3(std::max(1, zgrid)), dim3(256), 0, s>>>(image, (long long)image_doubles, dr, dc, dv,
                                                                                (long long)ncells, w, h, pitch, 0);
        HIP_TRY(hipGetLastError());
        if (ncells) {
            lp_variants_base_kernel<<<dim3(sgrid), dim3(256), 0, s>>>(image, (long long)image_doubles, dr, dc, dv, (long long)ncells,
                                                                      w, h, pitch, 1);
            HIP_TRY(hipGetLastError());
        }
        HIP_TRY(hipEventRecord(b->evb1, s)); // (read after the passes' waits: no wait of its own)
    }

    // a variant whose phase outran the history runs again from the image
    std::string text;
    QueueRun run;
    const int rc = run_queue(
        *b, b->q, kVarKernels, QueueText{"yalps_lpvar", true, "yalps_lpvar_solve", "variant"}, n,
        [&](int32_t i, int *iw, int *ih) { return *iw = w, *ih = h, checkCycles[i] != 0; },
        [&](VarLaunch &a) {
            a.desc = b->desc.as<const VarDesc>();
            a.w = w;
            a.h = h;
            a.aux_hbm = aux ? 1 : 0;
            a.image = b->image.as<const double>();
            a.prow = b->prow.as<const int32_t>();
            a.pcol = b->pcol.as<const int32_t>();
            a.pval = b->pval.as<const double>();
        },
        [] { return 0; },
        [&](const Launch &L, const std::string &kernel, int pass, int launch, long long hist_cap) {
            char line[256];
            std::snprintf(line, sizeof line, "launch=%d pass=%d kernel=%s class=%d aux=%d lps=%zu grid=%d lds=%zu hist_cap=%lld\n", launch,
                          pass, kernel.c_str(), L.cls, aux ? 1 : 0, L.items.size(), L.grid, L.shmem, hist_cap);
            text += line;
        },
        run);
    if (rc) return rc;
    float image_ms = 0.f;
    HIP_TRY(hipEventElapsedTime(&image_ms, b->evb0, b->evb1));
    b->info = "launches=" + std::to_string(run.launches) + " reruns=" + std::to_string(run.reruns.size()) + " rerun_lps=[" +
              join_ids(run.reruns) + "]" + " base_cells=" + std::to_string((long long)ncells) + " patch_cells=" + std::to_string(npatch) +
              " image_bytes=" + std::to_string(sizeof(double) * image_doubles) + "\n" + text;

    b->h_col0.resize(heven * n);
    b->h_pos.resize(perm * n);
    b->h_var.resize(perm * n);
    HIP_TRY(hipMemcpyAsync(b->h_col0.data(), b->q.col0.p, sizeof(double) * heven * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_pos.data(), b->q.pos.p, sizeof(int32_t) * perm * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_var.data(), b->q.var.p, sizeof(int32_t) * perm * n, hipMemcpyDeviceToHost, s));
    if (result_out) HIP_TRY(hipMemcpyAsync(result_out, b->q.result.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    if (pivots_out) HIP_TRY(hipMemcpyAsync(pivots_out, b->q.pivots.p, sizeof(int64_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (status_out) std::memcpy(status_out, b->q.h_status.data(), sizeof(int32_t) * n);
    if (gpu_ms_out) *gpu_ms_out = run.ms + image_ms;
    return 0;
}

void destroy_impl(yalps_lpvar *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    release(b->q);
    release({&b->desc, &b->brow, &b->bcol, &b->bval, &b->image, &b->prow, &b->pcol, &b->pval});
    if (b->evb0) (void)hipEventDestroy(b->evb0);
    if (b->evb1) (void)hipEventDestroy(b->evb1);
    close_device(*b);
    delete b;
}
} // namespace

extern "C" {

const char *yalps_lpvar_last_error(void) { return g_err.c_str(); }

int32_t yalps_lpvar_validate(int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row, const int32_t *base_col,
                             int32_t count, const int64_t *patch_offsets, const int32_t *patch_row, const int32_t *patch_col) {
    return validate(width, height, base_cells, base_row, base_col, count, patch_offsets, patch_row, patch_col);
}

int32_t yalps_lpvar_create(int32_t device, void *hip_stream, yalps_lpvar **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_lpvar_create: out is NULL");
    *out = nullptr;
    const int rc = create_impl(device, hip_stream, out);
    if (rc && *out) { // a half-made handle is taken down again and the reason kept
        const std::string why = g_err;
        destroy_impl(*out);
        *out = nullptr;
        g_err = why;
    }
    return rc;
}

void yalps_lpvar_destroy(yalps_lpvar *v) { destroy_impl(v); }

int32_t yalps_lpvar_solve(yalps_lpvar *v, int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row,
                          const int32_t *base_col, const double *base_val, int32_t count, const int64_t *patch_offsets,
                          const int32_t *patch_row, const int32_t *patch_col, const double *patch_val, const double *precision,
                          const double *maxPivots, const int32_t *checkCycles, int32_t keep_tableaux, int32_t *status_out,
                          double *result_out, int64_t *pivots_out, float *gpu_ms_out) {
    if (!v) return fail(YALPS_E_ARG, "yalps_lpvar_solve: handle is NULL");
    const int32_t rc = solve_impl(v, width, height, base_cells, base_row, base_col, base_val, count, patch_offsets, patch_row,
                                  patch_col, patch_val, precision, maxPivots, checkCycles, keep_tableaux, status_out, result_out,
                                  pivots_out, gpu_ms_out);
    if (rc) v->count = 0; // (no last solve to read from)
    return rc;
}

int32_t yalps_lpvar_solution(yalps_lpvar *v, int32_t i, double *col0, int32_t *positionOfVariable, int32_t *variableAtPosition) {
    if (!v || i < 0 || i >= v->count) return fail(YALPS_E_ARG, "yalps_lpvar_solution: no such variant in the last solve");
    const size_t h = (size_t)v->h, heven = (h + 1) & ~(size_t)1, np = (size_t)v->w + h;
    if (col0) std::memcpy(col0, v->h_col0.data() + (size_t)i * heven, sizeof(double) * h);
    if (positionOfVariable) std::memcpy(positionOfVariable, v->h_pos.data() + (size_t)i * np, sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, v->h_var.data() + (size_t)i * np, sizeof(int32_t) * np);
    return 0;
}

int32_t yalps_lpvar_tableau(yalps_lpvar *v, int32_t i, double *matrix) {
    if (!v || i < 0 || i >= v->count || !matrix) return fail(YALPS_E_ARG, "yalps_lpvar_tableau: no such variant in the last solve");
    if (!v->q.keep) return fail(YALPS_E_ARG, "yalps_lpvar_tableau: the last solve did not keep its tableaux (keep_tableaux)");
    const size_t wh = (size_t)v->w * (size_t)v->h;
    HIP_TRY(hipSetDevice(v->device));
    HIP_TRY(hipMemcpyAsync(matrix, v->q.tab.as<const double>() + (size_t)i * wh, sizeof(double) * wh, hipMemcpyDeviceToHost,
                           v->stream));
    HIP_TRY(hipStreamSynchronize(v->stream));
    return 0;
}

int32_t yalps_lpvar_info(const yalps_lpvar *v, char *buf, int32_t len) {
    if (!v || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_lpvar_info: bad argument");
    return info_out(v->info, buf, len);
}

} // extern "C"
