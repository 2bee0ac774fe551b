// lp_sens.hip -- libyalps_lpsens.so: a batch of independent LPs with their sensitivity ranges in one call (include/yalps_lpsens.h)
// C ABI + the lp_sens_kernel instantiations; the host side is lp_batch_host.inc on wg_queue_host.inc with this library's
// kernels, launch and names (LpSensLib).  A library of its own: nothing here is linked into the other four, and the pivot loop is
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
#include "wg_queue_host.inc"
#include "lp_batch_host.inc"

// the LP batch's host side around lp_sens_kernel: same limit, same size classes, same LDS bytes per class
static_assert(YALPS_LPSENS_MAX_BYTES == QUEUE_MAX_BYTES && YALPS_LPSENS_CLASSES == NCLASS, "include/yalps_lpsens.h");
const KernelTable<SensLaunch> kSensKernels = QUEUE_KERNEL_TABLE(lp_sens_kernel);
struct LpSensLib {
    using Launch = SensLaunch;
    static constexpr const char *name = "yalps_lpsens", *env = "YALPS_LPSENS";
    static constexpr bool sens = true;
    static const KernelTable<SensLaunch> &kernels() { return kSensKernels; }
};
} // namespace

struct yalps_lpsens : LpPass<LpSensLib> {};

extern "C" {

const char *yalps_lpsens_last_error(void) { return g_err.c_str(); }

int32_t yalps_lpsens_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *cell_offsets,
                              const int32_t *row, const int32_t *col) {
    return lp_validate<LpSensLib>(count, width, height, cell_offsets, row, col);
}

int32_t yalps_lpsens_create(int32_t device, void *hip_stream, yalps_lpsens **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_lpsens_create: out is NULL");
    return lp_create(device, hip_stream, out);
}

void yalps_lpsens_destroy(yalps_lpsens *b) { lp_destroy(b); }

int32_t yalps_lpsens_solve(yalps_lpsens *b, int32_t count, const int32_t *width, const int32_t *height,
                           const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                           const double *precision, const double *maxPivots, const int32_t *checkCycles,
                           int32_t keep_tableaux, int32_t *status_out, double *result_out, int64_t *pivots_out,
                           float *gpu_ms_out) {
    return lp_solve<LpSensLib>(b, "yalps_lpsens_solve", count, width, height, cell_offsets, row, col, val, precision, maxPivots,
                               checkCycles, keep_tableaux, status_out, result_out, pivots_out, gpu_ms_out);
}

int32_t yalps_lpsens_solution(yalps_lpsens *b, int32_t i, double *col0, int32_t *positionOfVariable,
                              int32_t *variableAtPosition) {
    return lp_solution<LpSensLib>(b, "yalps_lpsens_solution", i, col0, positionOfVariable, variableAtPosition);
}

int32_t yalps_lpsens_tableau(yalps_lpsens *b, int32_t i, double *matrix) {
    return lp_tableau<LpSensLib>(b, "yalps_lpsens_tableau", i, matrix);
}

int32_t yalps_lpsens_ranges(yalps_lpsens *b, int32_t i, double *row0, double *col_up, double *col_dn, double *row_lo,
                            double *row_hi) {
    if (!b || i < 0 || (size_t)i >= b->descs.size()) return fail(YALPS_E_ARG, "yalps_lpsens_ranges: no such LP in the last solve");
    if (b->q.h_status[(size_t)i] != YALPS_OPTIMAL)
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
    return info_out(b->info, buf, len);
}

} // extern "C"
