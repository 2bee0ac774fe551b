// lp_batch.hip -- libyalps_lpbatch.so: a batch of independent LPs in one call (include/yalps_lpbatch.h)
// C ABI + the lp_batch_kernel instantiations; the host side is lp_batch_host.inc on wg_queue_host.inc (shared with milp_batch.hip
// and lp_sens.hip).  A library of its own: nothing here is linked into libyalps_hip.so, and the pivot loop is that library's
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

#include "../../include/yalps_lpbatch.h"

#pragma clang fp contract(off)

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_batch_kernel.cuh"
#include "wg_queue_host.inc"
#include "lp_batch_host.inc"
} // namespace

#include "lp_batch_lib.inc"

extern "C" {

const char *yalps_lpbatch_last_error(void) { return g_err.c_str(); }

int32_t yalps_lpbatch_class(int32_t width, int32_t height) { return lp_class(width, height); }

int64_t yalps_lpbatch_lds_bytes(int32_t width, int32_t height) {
    return width < 1 || height < 1 ? -1 : (int64_t)small_lds_bytes(width, height);
}

int32_t yalps_lpbatch_aux_hbm(int32_t width, int32_t height) {
    return lp_class(width, height) < 0 ? -1 : (lp_class(width, height) == HBM_CLASS && lp_aux_hbm(width, height) ? 1 : 0);
}

int32_t yalps_lpbatch_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *cell_offsets,
                               const int32_t *row, const int32_t *col) {
    return lp_validate<LpBatchLib>(count, width, height, cell_offsets, row, col);
}

int32_t yalps_lpbatch_create(int32_t device, void *hip_stream, yalps_lpbatch **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_lpbatch_create: out is NULL");
    return lp_create(device, hip_stream, out);
}

void yalps_lpbatch_destroy(yalps_lpbatch *b) { lp_destroy(b); }

int32_t yalps_lpbatch_solve(yalps_lpbatch *b, int32_t count, const int32_t *width, const int32_t *height,
                            const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                            const double *precision, const double *maxPivots, const int32_t *checkCycles,
                            int32_t keep_tableaux, int32_t *status_out, double *result_out, int64_t *pivots_out,
                            float *gpu_ms_out) {
    return lp_solve<LpBatchLib>(b, "yalps_lpbatch_solve", count, width, height, cell_offsets, row, col, val, precision, maxPivots,
                                checkCycles, keep_tableaux, status_out, result_out, pivots_out, gpu_ms_out);
}

int32_t yalps_lpbatch_solution(yalps_lpbatch *b, int32_t i, double *col0, int32_t *positionOfVariable,
                               int32_t *variableAtPosition) {
    return lp_solution<LpBatchLib>(b, "yalps_lpbatch_solution", i, col0, positionOfVariable, variableAtPosition);
}

int32_t yalps_lpbatch_tableau(yalps_lpbatch *b, int32_t i, double *matrix) {
    return lp_tableau<LpBatchLib>(b, "yalps_lpbatch_tableau", i, matrix);
}

int32_t yalps_lpbatch_info(const yalps_lpbatch *b, char *buf, int32_t len) {
    if (!b || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_lpbatch_info: bad argument");
    return info_out(b->info, buf, len);
}

} // extern "C"
