// lp_warm.hip -- libyalps_lpwarm.so: many variants of one LP, each reoptimised from the base's optimal tableau (include/yalps_lpwarm.h)
// C ABI, host side and the lp_warm_kernel instantiations.  A library of its own: nothing here is linked into the others.
// The base's solve is libyalps_lpbatch.so's host code and kernels (lp_batch_host.inc, lp_batch_kernel.cuh) with one LP and
// its tableau kept, as milp_batch.hip's root pass; the variants' pass is wg_queue_host.inc with this library's kernel
// table; the pivot loop is libyalps_hip.so's wg_simplex.cuh, included unchanged.
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

#include "../../include/yalps_lpbatch.h"
#include "../../include/yalps_lpwarm.h"

#pragma clang fp contract(off)

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_batch_kernel.cuh"
#include "lp_warm_kernel.cuh"
#include "wg_queue_host.inc"
#include "lp_batch_host.inc"

static_assert(YALPS_LPWARM_MAX_BYTES == QUEUE_MAX_BYTES, "include/yalps_lpwarm.h");
const KernelTable<WarmLaunch> kWarmKernels = QUEUE_KERNEL_TABLE(lp_warm_kernel);
} // namespace

#include "lp_batch_lib.inc"

struct yalps_lpwarm {
    yalps_lpbatch *lp = nullptr; // the base's solve: device, stream, events, the kept final tableau
    QueueDevice dev;             // the same device and stream with the variants' class table (not owned)
    hipEvent_t evb0 = nullptr, evb1 = nullptr; // the image
    QueueBufs q;
    DevBuf desc, image, bpos, bvar, rec_p, rec_d;
    // the last solve
    int32_t w = 0, h = 0, count = 0;
    std::vector<double> h_col0;
    std::vector<int32_t> h_pos, h_var;
    std::string info;
};

namespace {
int validate(int64_t w, int64_t h, int64_t ncells, const int32_t *brow, const int32_t *bcol, int32_t count, const int64_t *off,
             const int32_t *prow, const int32_t *pcol) {
    if (w < 1 || h < 1) return fail(YALPS_E_ARG, "yalps_lpwarm: width and height must be at least 1");
    if (8 * w * h > YALPS_LPWARM_MAX_BYTES)
        return fail(YALPS_E_ARG, "yalps_lpwarm: tableau of " + std::to_string(8 * w * h) + " bytes is above the limit of " +
                                     std::to_string((long long)YALPS_LPWARM_MAX_BYTES));
    if (ncells < 0) return fail(YALPS_E_ARG, "yalps_lpwarm: base_cells < 0");
    if (ncells > 0 && (!brow || !bcol)) return fail(YALPS_E_ARG, "yalps_lpwarm: base_row / base_col is NULL");
    int64_t at = 0;
    if (int bad = check_cells(brow, bcol, 0, ncells, w, h, &at))
        return fail(YALPS_E_ARG, bad == 1 ? "yalps_lpwarm: base cell " + std::to_string(at) + " lies outside the tableau"
                                          : "yalps_lpwarm: base cells are not sorted by (row, col), strictly increasing");
    if (count < 0) return fail(YALPS_E_ARG, "yalps_lpwarm: count < 0");
    if (count == 0) return 0;
    if (!off) return fail(YALPS_E_ARG, "yalps_lpwarm: patch_offsets is NULL");
    if (off[0] < 0) return fail(YALPS_E_ARG, "yalps_lpwarm: variant 0: negative patch offset");
    for (int32_t i = 0; i < count; i++) {
        const std::string who = "yalps_lpwarm: variant " + std::to_string(i) + ": ";
        if (off[i + 1] < off[i]) return fail(YALPS_E_ARG, who + "patch offsets decrease");
        if (off[i + 1] > off[i] && (!prow || !pcol)) return fail(YALPS_E_ARG, who + "patch_row / patch_col is NULL");
        if (int bad = check_cells(prow, pcol, off[i], off[i + 1], w, h, &at))
            return fail(YALPS_E_ARG, bad == 1 ? who + "patch cell " + std::to_string(at) + " lies outside the tableau"
                                              : who + "patch cells are not sorted by (row, col), strictly increasing");
        for (int64_t c = off[i]; c < off[i + 1]; c++) {
            if (prow[c] > 0 && pcol[c] > 0)
                return fail(YALPS_E_ARG, who + "patch cell " + std::to_string(c - off[i]) + " lies in the body of the tableau (row > 0 and col > 0)");
            if (prow[c] == 0 && pcol[c] == 0)
                return fail(YALPS_E_ARG, who + "patch cell " + std::to_string(c - off[i]) + " is the cell (0, 0)");
        }
    }
    return 0;
}

int create_impl(yalps_lpwarm *b) {
    b->dev = *b->lp; // (stream and events stay the base pass's: one pass runs at a time)
    b->dev.own_stream = false;
    HIP_TRY(hipEventCreate(&b->evb0));
    HIP_TRY(hipEventCreate(&b->evb1));
    b->q.hist_first = std::max(1, env_int("YALPS_LPWARM_HIST", (int)HIST_FIRST)); // (test hook: forces the rerun)
    const int per_cu = env_int("YALPS_LPWARM_PER_CU", 0);                          // (test hook: one value for every class, a small grid)
    if (per_cu < 0 || per_cu > 8) return fail(YALPS_E_ARG, "YALPS_LPWARM_PER_CU: " + std::to_string(per_cu) + " is outside 1..8");
    const int cus = env_int("YALPS_LPWARM_CUS", 0);                                // (test hook: a grid smaller than the card)
    if (cus < 0) return fail(YALPS_E_ARG, "YALPS_LPWARM_CUS: " + std::to_string(cus) + " is negative");
    if (cus) b->dev.num_cus = std::min(cus, b->dev.num_cus);
    for (int k = 0; k < NCLASS; k++) {
        b->dev.lanes[k] = kClasses[k].lanes;
        b->dev.per_cu[k] = per_cu ? std::min(per_cu, kClasses[k].per_cu) : kClasses[k].per_cu;
    }
    b->info = "launches=0 reruns=0\n";
    return raise_lds_limit(kWarmKernels);
}

void destroy_impl(yalps_lpwarm *b) {
    if (!b) return;
    (void)hipSetDevice(b->lp->device);
    if (b->lp->stream) (void)hipStreamSynchronize(b->lp->stream);
    release(b->q);
    release({&b->desc, &b->image, &b->bpos, &b->bvar, &b->rec_p, &b->rec_d});
    if (b->evb0) (void)hipEventDestroy(b->evb0);
    if (b->evb1) (void)hipEventDestroy(b->evb1);
    lp_destroy(b->lp);
    delete b;
}

int solve_impl(yalps_lpwarm *b, int32_t w, int32_t h, int64_t ncells, const int32_t *brow, const int32_t *bcol, const double *bval,
               double bprecision, double bmaxPivots, int32_t bcheck, int32_t count, const int64_t *off, const int32_t *prow,
               const int32_t *pcol, const double *pval, const double *precision, const double *maxPivots, const int32_t *checkCycles,
               int32_t keep, int32_t *bstatus_out, double *bresult_out, int64_t *bpivots_out, int32_t *status_out, double *result_out,
               int64_t *pivots_out, float *gpu_ms_out) {
    if (int rc = validate(w, h, ncells, brow, bcol, count, off, prow, pcol)) return rc;
    if (ncells > 0 && !bval) return fail(YALPS_E_ARG, "yalps_lpwarm_solve: base_val is NULL");
    if (count > 0 && (!precision || !maxPivots || !checkCycles || (off[count] > off[0] && !pval)))
        return fail(YALPS_E_ARG, "yalps_lpwarm_solve: patch_val / precision / maxPivots / checkCycles is NULL");
    b->count = 0;
    b->q.keep = keep != 0;
    b->info = "launches=0 reruns=0\n";
    if (gpu_ms_out) *gpu_ms_out = 0.f;
    yalps_lpbatch *lp = b->lp;

    // the base: one LP through the LP batch's pass, its final matrix kept on the device
    int32_t bstatus = 0;
    double bresult = 0.0;
    int64_t bpivots = 0;
    float base_ms = 0.f;
    {
        const int64_t boff[2] = {0, ncells};
        if (int rc = lp_solve_impl(lp, 1, &w, &h, boff, brow, bcol, bval, &bprecision, &bmaxPivots, &bcheck, 1, &bstatus, &bresult,
                                   &bpivots, &base_ms)) {
            lp->descs.clear();
            return rc;
        }
    }
    if (bstatus_out) *bstatus_out = bstatus;
    if (bresult_out) *bresult_out = bresult;
    if (bpivots_out) *bpivots_out = bpivots;
    if (gpu_ms_out) *gpu_ms_out = base_ms;
    const std::string base_text = " base_status=" + std::to_string(bstatus) + " base_pivots=" + std::to_string((long long)bpivots);
    b->info = "launches=0 reruns=0 rerun_lps=[]" + base_text + "\n";
    if (bstatus != YALPS_OPTIMAL || count == 0) return 0;

    hipStream_t s = b->dev.stream;
    const size_t n = (size_t)count, heven = ((size_t)h + 1) & ~(size_t)1, perm = (size_t)w + (size_t)h;
    const int cls = lp_class(w, h);
    const bool lds = cls != HBM_CLASS, aux = !lds && lp_aux_hbm(w, h);
    const int pitch = lds ? small_lds_pitch(w - 1) : small_pcols(w - 1);
    const size_t image_doubles = (size_t)h * pitch + heven;

    // patch cells -> records (p, d): d against the base's initial cell, p through the base's final positionOfVariable
    const int32_t *bpos = lp->h_pos.data(); // (one LP: perm_off 0)
    std::vector<double> b_row0((size_t)w, 0.0), b_col0((size_t)h, 0.0);
    for (int64_t c = 0; c < ncells; c++) {
        if (brow[c] == 0) b_row0[(size_t)bcol[c]] = bval[c];
        if (bcol[c] == 0) b_col0[(size_t)brow[c]] = bval[c];
    }
    std::vector<WarmDesc> D(n);
    std::vector<int32_t> rec_p;
    std::vector<double> rec_d;
    rec_p.reserve((size_t)(off[count] - off[0]));
    rec_d.reserve((size_t)(off[count] - off[0]));
    for (size_t i = 0; i < n; i++) {
        WarmDesc &d = D[i];
        d.c0_lo = (long long)rec_p.size();
        for (int64_t c = off[i]; c < off[i + 1]; c++) // column 0, in patch order
            if (pcol[c] == 0) {
                const double delta = pval[c] - b_col0[(size_t)prow[c]];
                if (delta == 0.0) continue;
                rec_p.push_back(bpos[(size_t)w + (size_t)prow[c]]);
                rec_d.push_back(delta);
            }
        d.r0_lo = (long long)rec_p.size();
        for (int64_t c = off[i]; c < off[i + 1]; c++) // row 0, in patch order
            if (prow[c] == 0) {
                const double delta = pval[c] - b_row0[(size_t)pcol[c]];
                if (delta == 0.0) continue;
                rec_p.push_back(bpos[(size_t)pcol[c]]);
                rec_d.push_back(delta);
            }
        d.r0_hi = (long long)rec_p.size();
        d.precision = precision[i];
        d.max_pivots = maxPivots[i];
    }
    const size_t nrec = rec_p.size();
    for (size_t k = 0; k < nrec; k++) // (a permutation of 0 .. w+h-1 whose entry 0 is 0: nothing else can come back)
        if (rec_p[k] < 1 || (size_t)rec_p[k] >= perm || rec_p[k] == w)
            return fail(YALPS_E_DEVICE, "yalps_lpwarm_solve: the base's positionOfVariable is not a permutation");

    if (int rc = ensure(b->desc, sizeof(WarmDesc) * n)) return rc;
    if (int rc = ensure(b->image, sizeof(double) * image_doubles)) return rc;
    if (int rc = ensure(b->bpos, sizeof(int32_t) * perm)) return rc;
    if (int rc = ensure(b->bvar, sizeof(int32_t) * perm)) return rc;
    if (int rc = ensure(b->rec_p, sizeof(int32_t) * nrec)) return rc;
    if (int rc = ensure(b->rec_d, sizeof(double) * nrec)) return rc;
    if (int rc = ensure_outputs(b->q, n, heven * n, perm * n, (size_t)w * (size_t)h * n)) return rc;
    HIP_TRY(hipMemcpyAsync(b->desc.p, D.data(), sizeof(WarmDesc) * n, hipMemcpyHostToDevice, s));
    if (nrec) {
        HIP_TRY(hipMemcpyAsync(b->rec_p.p, rec_p.data(), sizeof(int32_t) * nrec, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->rec_d.p, rec_d.data(), sizeof(double) * nrec, hipMemcpyHostToDevice, s));
    }
    // (the base's permutations never left the device)
    HIP_TRY(hipMemcpyAsync(b->bpos.p, lp->q.pos.p, sizeof(int32_t) * perm, hipMemcpyDeviceToDevice, s));
    HIP_TRY(hipMemcpyAsync(b->bvar.p, lp->q.var.p, sizeof(int32_t) * perm, hipMemcpyDeviceToDevice, s));
    if (int rc = reset_status(b->q, s, n)) return rc;
    b->w = w;
    b->h = h;

    // the image, once per call: the kept matrix at this form's pitch; the solving launches follow on the same stream
    {
        const int grid = (int)std::min<size_t>((image_doubles + 255) / 256, (size_t)b->dev.num_cus * 8);
        HIP_TRY(hipEventRecord(b->evb0, s));
        lp_warm_image_kernel<<<dim3(std::max(1, grid)), dim3(256), 0, s>>>(b->image.as<double>(), (long long)image_doubles,
                                                                           lp->q.tab.as<const double>(), w, h, pitch);
        HIP_TRY(hipGetLastError());
        HIP_TRY(hipEventRecord(b->evb1, s)); // (read after the passes' waits: no wait of its own)
    }

    // a variant whose phase outran the history runs again from the image
    std::string text;
    QueueRun run;
    const int rc = run_queue(
        b->dev, b->q, kWarmKernels, QueueText{"yalps_lpwarm", true, "yalps_lpwarm_solve", "variant"}, n,
        [&](int32_t i, int *iw, int *ih) { return *iw = w, *ih = h, checkCycles[i] != 0; },
        [&](WarmLaunch &a) {
            a.desc = b->desc.as<const WarmDesc>();
            a.w = w;
            a.h = h;
            a.aux_hbm = aux ? 1 : 0;
            a.image = b->image.as<const double>();
            a.bpos = b->bpos.as<const int32_t>();
            a.bvar = b->bvar.as<const int32_t>();
            a.rec_p = b->rec_p.as<const int32_t>();
            a.rec_d = b->rec_d.as<const double>();
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
              join_ids(run.reruns) + "]" + base_text + " patch_cells=" + std::to_string((long long)(off[count] - off[0])) +
              " records=" + std::to_string(nrec) + " image_bytes=" + std::to_string(sizeof(double) * image_doubles) + "\n" + text;

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
    if (gpu_ms_out) *gpu_ms_out = base_ms + image_ms + run.ms;
    b->count = count;
    return 0;
}
} // namespace

extern "C" {

const char *yalps_lpwarm_last_error(void) { return g_err.c_str(); }

int32_t yalps_lpwarm_validate(int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row, const int32_t *base_col,
                              int32_t count, const int64_t *patch_offsets, const int32_t *patch_row, const int32_t *patch_col) {
    return validate(width, height, base_cells, base_row, base_col, count, patch_offsets, patch_row, patch_col);
}

int32_t yalps_lpwarm_create(int32_t device, void *hip_stream, yalps_lpwarm **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_lpwarm_create: out is NULL");
    *out = nullptr;
    yalps_lpbatch *lp = nullptr;
    if (int rc = lp_create(device, hip_stream, &lp)) return rc;
    yalps_lpwarm *b = new yalps_lpwarm();
    b->lp = lp;
    if (int rc = create_impl(b)) { // a half-made handle is taken down again and the reason kept
        const std::string why = g_err;
        destroy_impl(b);
        g_err = why;
        return rc;
    }
    *out = b;
    return 0;
}

void yalps_lpwarm_destroy(yalps_lpwarm *v) { destroy_impl(v); }

int32_t yalps_lpwarm_solve(yalps_lpwarm *v, int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row,
                           const int32_t *base_col, const double *base_val, double base_precision, double base_maxPivots,
                           int32_t base_checkCycles, int32_t count, const int64_t *patch_offsets, const int32_t *patch_row,
                           const int32_t *patch_col, const double *patch_val, const double *precision, const double *maxPivots,
                           const int32_t *checkCycles, int32_t keep_tableaux, int32_t *base_status_out, double *base_result_out,
                           int64_t *base_pivots_out, int32_t *status_out, double *result_out, int64_t *pivots_out, float *gpu_ms_out) {
    if (!v) return fail(YALPS_E_ARG, "yalps_lpwarm_solve: handle is NULL");
    const int32_t rc = solve_impl(v, width, height, base_cells, base_row, base_col, base_val, base_precision, base_maxPivots,
                                  base_checkCycles, count, patch_offsets, patch_row, patch_col, patch_val, precision, maxPivots,
                                  checkCycles, keep_tableaux, base_status_out, base_result_out, base_pivots_out, status_out, result_out,
                                  pivots_out, gpu_ms_out);
    if (rc) v->count = 0; // (no last solve to read from)
    return rc;
}

int32_t yalps_lpwarm_solution(yalps_lpwarm *v, int32_t i, double *col0, int32_t *positionOfVariable, int32_t *variableAtPosition) {
    if (!v || i < 0 || i >= v->count) return fail(YALPS_E_ARG, "yalps_lpwarm_solution: no such variant in the last solve");
    const size_t h = (size_t)v->h, heven = (h + 1) & ~(size_t)1, np = (size_t)v->w + h;
    if (col0) std::memcpy(col0, v->h_col0.data() + (size_t)i * heven, sizeof(double) * h);
    if (positionOfVariable) std::memcpy(positionOfVariable, v->h_pos.data() + (size_t)i * np, sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, v->h_var.data() + (size_t)i * np, sizeof(int32_t) * np);
    return 0;
}

int32_t yalps_lpwarm_tableau(yalps_lpwarm *v, int32_t i, double *matrix) {
    if (!v || i < 0 || i >= v->count || !matrix) return fail(YALPS_E_ARG, "yalps_lpwarm_tableau: no such variant in the last solve");
    if (!v->q.keep) return fail(YALPS_E_ARG, "yalps_lpwarm_tableau: the last solve did not keep its tableaux (keep_tableaux)");
    const size_t wh = (size_t)v->w * (size_t)v->h;
    HIP_TRY(hipSetDevice(v->dev.device));
    HIP_TRY(hipMemcpyAsync(matrix, v->q.tab.as<const double>() + (size_t)i * wh, sizeof(double) * wh, hipMemcpyDeviceToHost,
                           v->dev.stream));
    HIP_TRY(hipStreamSynchronize(v->dev.stream));
    return 0;
}

int32_t yalps_lpwarm_info(const yalps_lpwarm *v, char *buf, int32_t len) {
    if (!v || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_lpwarm_info: bad argument");
    return info_out(v->info, buf, len);
}

} // extern "C"
