/*
 * yalps_lpbatch.h -- C ABI of libyalps_lpbatch.so: many independent small LPs in one call (MI355X, gfx950).
 *
 * yalps_hip.h solves one model per call.  A batch here is `count` unrelated LPs of different shapes, each given as
 * the cells `tableauModel` writes into its zeroed matrix (reference src/tableau.ts:87-134) -- (row, col, val) sorted by
 * (row, col), strictly increasing, column 0 = RHS column, row 0 = objective row: the contract of yalps_tableau_assemble.
 * Every LP is assembled on the device with identity permutations and solved by `simplex(tableau, options)`
 * (src/simplex.ts:106-144) with its own precision, maxPivots and checkCycles, one workgroup per LP.
 *
 * Return protocol as yalps_hip.h: the YALPS_* codes below, negative = native failure with text through
 * yalps_lpbatch_last_error() (per thread).  There is NO CPU fallback: without a usable gfx950 device
 * yalps_lpbatch_create fails with YALPS_E_DEVICE.  A handle belongs to one thread at a time; its device buffers are
 * kept and grown between calls.
 *
 * Size limit: an LP's tableau (8 * width * height bytes) may not exceed YALPS_LPBATCH_MAX_BYTES; larger models are
 * the business of yalps_hip.h's whole-chip kernels.
 */
#ifndef YALPS_LPBATCH_H
#define YALPS_LPBATCH_H

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

#define YALPS_LPBATCH_MAX_BYTES (4 << 20)
#define YALPS_LPBATCH_CLASSES 5 /* size classes 0..3: the LDS form, by LDS bytes; 4: the HBM form */

typedef struct yalps_lpbatch yalps_lpbatch;

const char *yalps_lpbatch_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream. */
int32_t yalps_lpbatch_create(int32_t device, void *hip_stream, yalps_lpbatch **out);
void yalps_lpbatch_destroy(yalps_lpbatch *b);

/* Host only (no device needed).  The size class of a width x height LP: 0..3 = the LDS form (the class bounds its LDS
 * bytes, which yalps_lpbatch_lds_bytes returns), 4 = the HBM form, -1 = above YALPS_LPBATCH_MAX_BYTES or a bad size. */
int32_t yalps_lpbatch_class(int32_t width, int32_t height);
int64_t yalps_lpbatch_lds_bytes(int32_t width, int32_t height);
/* Host only.  1 where a width x height LP is solved in the aux form of the HBM class: its pivot column and pivot row buffers
 * (even(width - 1) + height doubles) are above 64 KiB, that is even(width - 1) + height > 8192, and live behind the tableau
 * in the HBM workspace instead of LDS.  0 for every other batchable LP, -1 where yalps_lpbatch_class returns -1. */
int32_t yalps_lpbatch_aux_hbm(int32_t width, int32_t height);
/* Host only: what yalps_lpbatch_solve checks before it touches the device.  0, or YALPS_E_ARG with the index of the
 * first offending LP in the error text: width < 1, height < 1, a tableau above YALPS_LPBATCH_MAX_BYTES, cell offsets
 * that decrease, a cell outside the tableau, cells not strictly increasing by (row, col). */
int32_t yalps_lpbatch_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *cell_offsets,
                               const int32_t *row, const int32_t *col);

/* Solves LPs 0 .. count-1.  Cells of LP i: entries [cell_offsets[i], cell_offsets[i + 1]) of row / col / val.
 * precision / maxPivots (may be +Infinity) / checkCycles are per LP.  keep_tableaux != 0 also keeps every final matrix
 * on the device for yalps_lpbatch_tableau.  status_out (YALPS_OPTIMAL .. YALPS_CYCLED), result_out (rounded M[0,0] |
 * entering column | NaN) and pivots_out are per LP and may be NULL; gpu_ms_out (optional) = HIP-event time of the
 * kernels.  count == 0 succeeds and launches nothing.  Returns 0 or a negative error; nothing is launched when an
 * argument is refused. */
int32_t yalps_lpbatch_solve(yalps_lpbatch *b, int32_t count, const int32_t *width, const int32_t *height,
                            const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                            const double *precision, const double *maxPivots, const int32_t *checkCycles,
                            int32_t keep_tableaux, int32_t *status_out, double *result_out, int64_t *pivots_out,
                            float *gpu_ms_out);

/* LP i of the last solve, what solution() reads (src/YALPS.ts:18-19,32): column 0 (height doubles) and both
 * permutations (width + height int32 each).  NULL pointers are skipped. */
int32_t yalps_lpbatch_solution(yalps_lpbatch *b, int32_t i, double *col0, int32_t *positionOfVariable,
                               int32_t *variableAtPosition);
/* LP i of the last solve: the whole final matrix, row-major width * height.  Needs keep_tableaux. */
int32_t yalps_lpbatch_tableau(yalps_lpbatch *b, int32_t i, double *matrix);
/* Text about the last solve: launches made, per launch the kernel's spelling, its size class, LP count, grid and LDS
 * bytes, and the LPs rerun because their checkCycles history overflowed.  Writes at most len - 1 characters and returns the
 * length of the whole text: a return value >= len means the text was cut (call again with a larger buffer). */
int32_t yalps_lpbatch_info(const yalps_lpbatch *b, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_LPBATCH_H */
