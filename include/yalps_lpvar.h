/*
 * yalps_lpvar.h -- C ABI of libyalps_lpvar.so: many variants of ONE LP in one call (MI355X, gfx950).
 *
 * yalps_lpbatch.h solves `count` unrelated LPs, each shipped as all of its cells.  Here the LPs of a call share one
 * tableau: the *base*, given once as the cells `tableauModel` writes into its zeroed matrix (reference
 * src/tableau.ts:87-134) -- (row, col, val) sorted by (row, col), strictly increasing, column 0 = RHS column, row 0 =
 * objective row: the contract of yalps_tableau_assemble -- and every variant is a *patch*, a short list of cells in the
 * same form that is written over the base.  A patch cell may hit a cell the base has or one it does not; an empty
 * patch is the base itself.  Variant i is the tableau `base with patch i on top`, identity permutations, solved by
 * `simplex(tableau, options)` (src/simplex.ts:106-144) with its own precision, maxPivots and checkCycles by one
 * workgroup -- bit for bit what yalps_lpbatch_solve computes from that tableau's full cell list.
 *
 * On the device the base is assembled once per call into a dense image; every variant starts from a copy of the image
 * instead of a zero pass and a scatter of all cells, and only the patches cross PCIe.
 *
 * Return protocol as yalps_lpbatch.h: the YALPS_* codes below, negative = native failure with text through
 * yalps_lpvar_last_error() (per thread).  There is NO CPU fallback: without a usable gfx950 device yalps_lpvar_create
 * fails with YALPS_E_DEVICE.  A handle belongs to one thread at a time; its device buffers are kept and grown between
 * calls.
 *
 * Size limit: the tableau (8 * width * height bytes) may not exceed YALPS_LPVAR_MAX_BYTES.
 */
#ifndef YALPS_LPVAR_H
#define YALPS_LPVAR_H

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

#define YALPS_LPVAR_MAX_BYTES (4 << 20)

typedef struct yalps_lpvar yalps_lpvar;

const char *yalps_lpvar_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream. */
int32_t yalps_lpvar_create(int32_t device, void *hip_stream, yalps_lpvar **out);
void yalps_lpvar_destroy(yalps_lpvar *v);

/* Host only: what yalps_lpvar_solve checks before it touches the device.  0, or YALPS_E_ARG: width < 1, height < 1, a
 * tableau above YALPS_LPVAR_MAX_BYTES, a base cell outside the tableau or base cells not strictly increasing by
 * (row, col); and, with the index of the first offending variant in the error text, patch offsets that decrease, a
 * patch cell outside the tableau, patch cells not strictly increasing by (row, col). */
int32_t yalps_lpvar_validate(int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row,
                             const int32_t *base_col, int32_t count, const int64_t *patch_offsets,
                             const int32_t *patch_row, const int32_t *patch_col);

/* Solves variants 0 .. count-1 of the width x height base.  Patch of variant i: entries [patch_offsets[i],
 * patch_offsets[i + 1]) of patch_row / patch_col / patch_val.  precision / maxPivots (may be +Infinity) / checkCycles are
 * per variant.  keep_tableaux != 0 also keeps every final matrix on the device for yalps_lpvar_tableau.  status_out
 * (YALPS_OPTIMAL .. YALPS_CYCLED), result_out (rounded M[0,0] | entering column | NaN) and pivots_out are per variant and
 * may be NULL; gpu_ms_out (optional) = HIP-event time of the kernels, the image's assembly included.  count == 0 succeeds
 * and launches nothing.  Returns 0 or a negative error; nothing is launched when an argument is refused. */
int32_t yalps_lpvar_solve(yalps_lpvar *v, int32_t width, int32_t height, int64_t base_cells, const int32_t *base_row,
                          const int32_t *base_col, const double *base_val, int32_t count, const int64_t *patch_offsets,
                          const int32_t *patch_row, const int32_t *patch_col, const double *patch_val,
                          const double *precision, const double *maxPivots, const int32_t *checkCycles,
                          int32_t keep_tableaux, int32_t *status_out, double *result_out, int64_t *pivots_out,
                          float *gpu_ms_out);

/* Variant i of the last solve, what solution() reads (src/YALPS.ts:18-19,32): column 0 (height doubles) and both
 * permutations (width + height int32 each).  NULL pointers are skipped. */
int32_t yalps_lpvar_solution(yalps_lpvar *v, int32_t i, double *col0, int32_t *positionOfVariable,
                             int32_t *variableAtPosition);
/* Variant i of the last solve: the whole final matrix, row-major width * height.  Needs keep_tableaux. */
int32_t yalps_lpvar_tableau(yalps_lpvar *v, int32_t i, double *matrix);
/* Text about the last solve.  First line: launches of the solving kernel, variants rerun because their checkCycles
 * history overflowed (and which), the base's and the patches' cell counts, the image's bytes.  Then per launch the
 * kernel's spelling, the size class (0..3 the LDS form, 4 the HBM form), whether it ran in the aux form of the HBM class
 * (pivot column and pivot row buffers behind the tableau in HBM), variant count, grid and LDS bytes.  Writes at most
 * len - 1 characters and returns the length of the whole text: a return value >= len means the text was cut. */
int32_t yalps_lpvar_info(const yalps_lpvar *v, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_LPVAR_H */
