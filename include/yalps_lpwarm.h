/*
 * yalps_lpwarm.h -- C ABI of libyalps_lpwarm.so: many variants of ONE LP, each reoptimised from the base's optimal
 * tableau (MI355X, gfx950).
 *
 * yalps_lpvar.h solves every variant from the *initial* tableau `base with patch on top`.  Here the base is solved once,
 * and a variant whose patch touches only column 0 (right-hand sides) and row 0 (objective coefficients) of the initial
 * tableau starts from the base's FINAL tableau F and its permutations, updated for the patch -- the body of F stays
 * valid, only its column 0 and row 0 change -- and `simplex(tableau, options)` (reference src/simplex.ts:106-144) runs
 * from there unchanged: phase 1 repairs a right-hand side that went negative, phase 2 continues, as after `applyCuts`
 * (src/branchAndCut.ts:22-61).
 *
 * The warm tableau, exactly (w = width, pos = the base's final positionOfVariable, b0 = the base's initial tableau, 0
 * where no cell was written, d = patch value - b0[cell]; cells with d == 0.0 are dropped; every product and every sum
 * is rounded on its own):
 *   1. column 0 cells (r, 0), r >= 1, in patch order, p = pos[w + r]:
 *        p < w:  W[i,0] = W[i,0] + d * W[i,p] for every row i, row 0 included;   else:  W[p-w,0] += d
 *   2. row 0 cells (0, c), c >= 1, in patch order, on the column 0 step 1 left, p = pos[c]:
 *        p < w:  W[0,p] += d;   else:  W[0,j] = W[0,j] - d * W[p-w,j] for every column j, column 0 included
 * Variant i is `simplex` on that tableau with the base's permutations and its own precision, maxPivots and checkCycles,
 * which count the reoptimisation's pivots alone.  Its answer is a valid answer for the variant's LP, not necessarily
 * the vertex a solve from the initial tableau ends in.
 *
 * Cells, return protocol, handles and the size limit are yalps_lpvar.h's: base cells sorted by (row, col), strictly
 * increasing; the YALPS_* codes below, negative = native failure with text through yalps_lpwarm_last_error() (per
 * thread); NO CPU fallback; a handle belongs to one thread at a time.
 */
#ifndef YALPS_LPWARM_H
#define YALPS_LPWARM_H

#include <stdint.h>

#ifdef __cplusplus
extern "C" {
#endif

#ifndef YALPS_OPTIMAL
#define YALPS_OPTIMAL 0
#define YALPS_INFEASIBLE 1
#define YALPS_UNBOUNDED 2
#define YALPS_CYCLED 3
#define YALPS_E_ARG (-1)    /* bad argument */
#define YALPS_E_DEVICE (-2) /* no usable HIP device / HIP runtime error */
#define YALPS_E_NOMEM (-3)  /* device or host allocation failed */
#endif

#define YALPS_LPWARM_MAX_BYTES (4 << 20)

typedef struct yalps_lpwarm yalps_lpwarm;

const char *yalps_lpwarm_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream. */
int32_t yalps_lpwarm_create(int32_t device, void *hip_stream, yalps_lpwarm **out);
void yalps_lpwarm_destroy(yalps_lpwarm *v);

/* Host only: what yalps_lpwarm_solve checks before it touches the device.  0, or YALPS_E_ARG: everything
 * yalps_lpvar_validate refuses, and, with the index of the first offending variant in the error text, a patch cell in
 * the body of the tableau (row > 0 and col > 0) and the cell (0, 0). */
int32_t yalps_lpwarm_validate(int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row,
                              const int32_t *base_col, int32_t count, const int64_t *patch_offsets,
                              const int32_t *patch_row, const int32_t *patch_col);

/* Solves the width x height base with base_precision / base_maxPivots / base_checkCycles, then reoptimises variants
 * 0 .. count-1 from its final tableau.  Patch of variant i: entries [patch_offsets[i], patch_offsets[i + 1]) of
 * patch_row / patch_col / patch_val, cells of the INITIAL tableau in row 0 or column 0, never (0, 0).  precision /
 * maxPivots (may be +Infinity) / checkCycles are per variant.  keep_tableaux != 0 also keeps every variant's final
 * matrix on the device for yalps_lpwarm_tableau.  base_status_out / base_result_out / base_pivots_out: the base's solve.
 * Where the base does not end YALPS_OPTIMAL nothing is launched for the variants, the per-variant outputs are not
 * written, there is no variant to read afterwards, and the call still returns 0.  status_out (YALPS_OPTIMAL ..
 * YALPS_CYCLED), result_out (rounded M[0,0] | entering column | NaN) and pivots_out (of the reoptimisation alone) are per
 * variant; every output pointer may be NULL.  gpu_ms_out (optional) = HIP-event time of the kernels, the base's solve
 * and the image included.  Returns 0 or a negative error; nothing is launched when an argument is refused. */
int32_t yalps_lpwarm_solve(yalps_lpwarm *v, int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row,
                           const int32_t *base_col, const double *base_val, double base_precision, double base_maxPivots,
                           int32_t base_checkCycles, int32_t count, const int64_t *patch_offsets, const int32_t *patch_row,
                           const int32_t *patch_col, const double *patch_val, const double *precision,
                           const double *maxPivots, const int32_t *checkCycles, int32_t keep_tableaux,
                           int32_t *base_status_out, double *base_result_out, int64_t *base_pivots_out,
                           int32_t *status_out, double *result_out, int64_t *pivots_out, float *gpu_ms_out);

/* Variant i of the last solve, what solution() reads (src/YALPS.ts:18-19,32): column 0 (height doubles) and both
 * permutations (width + height int32 each).  NULL pointers are skipped. */
int32_t yalps_lpwarm_solution(yalps_lpwarm *v, int32_t i, double *col0, int32_t *positionOfVariable,
                              int32_t *variableAtPosition);
/* Variant i of the last solve: the whole final matrix, row-major width * height.  Needs keep_tableaux. */
int32_t yalps_lpwarm_tableau(yalps_lpwarm *v, int32_t i, double *matrix);
/* Text about the last solve.  First line: launches of lp_warm_kernel, variants rerun because their checkCycles history
 * overflowed (and which), base_status, base_pivots, the patches' cells, the records made of them (cells whose value
 * does not differ from the base's are dropped), the image's bytes.  Then per launch of lp_warm_kernel the kernel's
 * spelling, the size class (0..3 the LDS form, 4 the HBM form), aux, variant count, grid and LDS bytes, as
 * yalps_lpvar_info.  Writes at most len - 1 characters and returns the length of the whole text. */
int32_t yalps_lpwarm_info(const yalps_lpwarm *v, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_LPWARM_H */
