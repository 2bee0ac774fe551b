// lp_sens.hip -- libyalps_lpsens.so: a batch of independent LPs with their sensitivity ranges in one call (include/yalps_lpsens.h)
// C ABI + the lp_sens_kernel instantiations; the host side is lp_batch_host.inc, compiled here a third time with this library's
// kernel, handle and names.  A library of its own: nothing here is linked into the other four, and the pivot loop is
// wg_simplex.cuh, included unchanged.
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

#include "../../include/yalps_lpsens.h"

#pragma clang fp contract(off)

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_sens_kernel.cuh"
} // namespace

// lp_batch_host.inc around lp_sens_kernel: same limit, same size classes, same LDS bytes per class
#define LPB_KERNEL lp_sens_kernel
#define LPB_KERNEL_NAME "lp_sens_kernel"
#define LPB_NAME "yalps_lpsens"
#define LPB_ENV "YALPS_LPSENS"
#define LPB_SENS 1
#define yalps_lpbatch yalps_lpsens
#define YALPS_LPBATCH_MAX_BYTES YALPS_LPSENS_MAX_BYTES
#define YALPS_LPBATCH_CLASSES YALPS_LPSENS_CLASSES
#include "lp_batch_host.inc"
#undef yalps_lpbatch

extern "C" {

const char *yalps_lpsens_last_error(void) { return g_err.c_str(); }

int32_t yalps_lpsens_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *cell_offsets,
                              const int32_t *row, const int32_t *col) {
    return validate(count, width, height, cell_offsets, row, col);
}

int32_t yalps_lpsens_create(int32_t device, void *hip_stream, yalps_lpsens **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_lpsens_create: out is NULL");
    return lpbatch_create(device, hip_stream, out);
}

void yalps_lpsens_destroy(yalps_lpsens *b) { lpbatch_destroy_impl(b); }

int32_t yalps_lpsens_solve(yalps_lpsens *b, int32_t count, const int32_t *width, const int32_t *height,
                           const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                           const double *precision, const double *maxPivots, const int32_t *checkCycles,
                           int32_t keep_tableaux, int32_t *status_out, double *result_out, int64_t *pivots_out,
                           float *gpu_ms_out) {
    if (!b) return fail(YALPS_E_ARG, "yalps_lpsens_solve: handle is NULL");
    const int32_t rc = solve_impl(b, count, width, height, cell_offsets, row, col, val, precision, maxPivots, checkCycles,
                                  keep_tableaux, status_out, result_out, pivots_out, gpu_ms_out);
    if (rc) b->descs.clear(); // (no last solve to read from)
    return rc;
}

int32_t yalps_lpsens_solution(yalps_lpsens *b, int32_t i, double *col0, int32_t *positionOfVariable,
                              int32_t *variableAtPosition) {
    if (!b || i < 0 || (size_t)i >= b->descs.size()) return fail(YALPS_E_ARG, "yalps_lpsens_solution: no such LP in the last solve");
    const LpDesc &d = b->descs[(size_t)i];
    const size_t np = (size_t)d.w + (size_t)d.h;
    if (col0) std::memcpy(col0, b->h_col0.data() + d.col0_off, sizeof(double) * (size_t)d.h);
    if (positionOfVariable) std::memcpy(positionOfVariable, b->h_pos.data() + d.perm_off, sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, b->h_var.data() + d.perm_off, sizeof(int32_t) * np);
    return 0;
}

int32_t yalps_lpsens_tableau(yalps_lpsens *b, int32_t i, double *matrix) {
    if (!b || i < 0 || (size_t)i >= b->descs.size() || !matrix)
        return fail(YALPS_E_ARG, "yalps_lpsens_tableau: no such LP in the last solve");
    if (!b->keep) return fail(YALPS_E_ARG, "yalps_lpsens_tableau: the last solve did not keep its tableaux (keep_tableaux)");
    const LpDesc &d = b->descs[(size_t)i];
    HIP_TRY(hipSetDevice(b->device));
    HIP_TRY(hipMemcpyAsync(matrix, static_cast<const double *>(b->tab.p) + d.tab_off, sizeof(double) * (size_t)d.w * (size_t)d.h,
                           hipMemcpyDeviceToHost, b->stream));
    HIP_TRY(hipStreamSynchronize(b->stream));
    return 0;
}

int32_t yalps_lpsens_ranges(yalps_lpsens *b, int32_t i, double *row0, double *col_up, double *col_dn, double *row_lo,
                            double *row_hi) {
    if (!b || i < 0 || (size_t)i >= b->descs.size()) return fail(YALPS_E_ARG, "yalps_lpsens_ranges: no such LP in the last solve");
    if (b->h_status[(size_t)i] != YALPS_OPTIMAL)
        return fail(YALPS_E_ARG, "yalps_lpsens_ranges: LP " + std::to_string(i) + " did not end optimal: it has no ranges");
    const LpDesc &d = b->descs[(size_t)i];
    const size_t w = (size_t)d.w, h = (size_t)d.h;
    const double *s = b->h_sens.data() + 3 * d.perm_off; // row0[w] col_up[w] col_dn[w] row_lo[h] row_hi[h]
    if (row0) std::memcpy(row0, s, sizeof(double) * w);
    if (col_up) std::memcpy(col_up, s + w, sizeof(double) * w);
    if (col_dn) std::memcpy(col_dn, s + 2 * w, sizeof(double) * w);
    if (row_lo) std::memcpy(row_lo, s + 3 * w, sizeof(double) * h);
    if (row_hi) std::memcpy(row_hi, s + 3 * w + h, sizeof(double) * h);
    return 0;
}

int32_t yalps_lpsens_info(const yalps_lpsens *b, char *buf, int32_t len) {
    if (!b || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_lpsens_info: bad argument");
    const size_t n = std::min(b->info.size(), (size_t)len - 1);
    std::memcpy(buf, b->info.data(), n);
    buf[n] = 0;
    return (int32_t)std::min<size_t>(b->info.size(), INT32_MAX); // (the whole text's length: >= len means it was cut)
}

} // extern "C"
