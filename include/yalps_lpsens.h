/*
 * yalps_lpsens.h -- C ABI of libyalps_lpsens.so: many independent small LPs in one call, each with what its final
 * tableau says about its sensitivity (MI355X, gfx950).
 *
 * The batch is that of yalps_lpbatch.h: `count` unrelated LPs of different shapes, each given as the cells `tableauModel`
 * writes into its zeroed matrix (reference src/tableau.ts:87-134) -- (row, col, val) sorted by (row, col), strictly
 * increasing, column 0 = RHS column, row 0 = objective row.  Every LP is assembled on the device and solved by
 * `simplex(tableau, options)` (src/simplex.ts:106-144), one workgroup per LP; status, result, pivot count, column 0,
 * permutations and kept matrix are bit for bit those of yalps_lpbatch_solve.  For an LP that ends "optimal" the same
 * workgroup then ranges the final matrix M in place (p = the LP's precision):
 *
 *   row0[c]   = M[0,c]                                                   c = 0 .. width-1
 *   col_up[c] = min{ M[r,0] /  M[r,c] : 1 <= r < height, M[r,c] >  p }   c = 1 .. width-1
 *   col_dn[c] = min{ M[r,0] / -M[r,c] : 1 <= r < height, M[r,c] < -p }
 *   row_lo[r] = max{ M[0,c] /  M[r,c] : 1 <= c < width,  M[r,c] >  p }   r = 1 .. height-1
 *   row_hi[r] = min{ M[0,c] /  M[r,c] : 1 <= c < width,  M[r,c] < -p }
 *
 * An empty set gives +Infinity (row_lo: -Infinity); entry 0 of the four ratio arrays is 0.0; every quotient is one IEEE
 * division and a NaN quotient is ignored.  Row 0 holds the reduced costs and the duals; col_up / col_dn say how far the
 * non-basic variable of a column can move in either direction before a basic variable reaches zero (the right-hand-side
 * range of a constraint whose slack it is); row_lo / row_hi say how far the objective coefficient of the basic variable
 * of a row can move before a reduced cost changes sign.  Nothing is clamped or signed here: yalps_amd/sensitivity.py maps
 * the arrays to a model's duals, reduced costs and ranges.
 *
 * Return protocol, size limit (YALPS_LPSENS_MAX_BYTES per tableau), size classes and LDS bytes per class: those of
 * yalps_lpbatch.h.  There is NO CPU fallback: without a usable gfx950 device yalps_lpsens_create fails with
 * YALPS_E_DEVICE.  A handle belongs to one thread at a time; its device buffers are kept and grown between calls.
 */
#ifndef YALPS_LPSENS_H
#define YALPS_LPSENS_H

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

#define YALPS_LPSENS_MAX_BYTES (4 << 20)
#define YALPS_LPSENS_CLASSES 5 /* size classes 0..3: the LDS form, by LDS bytes; 4: the HBM form */

typedef struct yalps_lpsens yalps_lpsens;

const char *yalps_lpsens_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream. */
int32_t yalps_lpsens_create(int32_t device, void *hip_stream, yalps_lpsens **out);
void yalps_lpsens_destroy(yalps_lpsens *b);

/* Host only: what yalps_lpsens_solve checks before it touches the device.  0, or YALPS_E_ARG with the index of the
 * first offending LP in the error text (the checks of yalps_lpbatch_validate). */
int32_t yalps_lpsens_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *cell_offsets,
                              const int32_t *row, const int32_t *col);

/* Solves LPs 0 .. count-1 and ranges those that end optimal.  Arguments and outputs as yalps_lpbatch_solve. */
int32_t yalps_lpsens_solve(yalps_lpsens *b, int32_t count, const int32_t *width, const int32_t *height,
                           const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                           const double *precision, const double *maxPivots, const int32_t *checkCycles,
                           int32_t keep_tableaux, int32_t *status_out, double *result_out, int64_t *pivots_out,
                           float *gpu_ms_out);

/* LP i of the last solve: column 0 (height doubles) and both permutations (width + height int32 each).  NULL pointers
 * are skipped. */
int32_t yalps_lpsens_solution(yalps_lpsens *b, int32_t i, double *col0, int32_t *positionOfVariable,
                              int32_t *variableAtPosition);
/* LP i of the last solve: the whole final matrix, row-major width * height.  Needs keep_tableaux. */
int32_t yalps_lpsens_tableau(yalps_lpsens *b, int32_t i, double *matrix);
/* LP i of the last solve, which must have ended YALPS_OPTIMAL (YALPS_E_ARG otherwise: nothing was written for it):
 * row0, col_up, col_dn (width doubles each) and row_lo, row_hi (height doubles each).  NULL pointers are skipped. */
int32_t yalps_lpsens_ranges(yalps_lpsens *b, int32_t i, double *row0, double *col_up, double *col_dn, double *row_lo,
                            double *row_hi);
/* Text about the last solve, in the format of yalps_lpbatch_info; the kernel is spelled lp_sens_kernel<T[,check][,lds]>. */
int32_t yalps_lpsens_info(const yalps_lpsens *b, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_LPSENS_H */
