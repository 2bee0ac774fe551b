/*
 * yalps_lpdense.h -- C ABI of libyalps_lpdense.so: a batch of dense LPs of one shape, read from and answered in DEVICE
 * memory (MI355X, gfx950).
 *
 * yalps_lpbatch.h takes every LP as a packed cell list in host memory.  Here the `count` LPs of a call share one shape
 * and lie in device memory as dense operands, scipy's linprog form with x >= 0:
 *     maximize | minimize  c . x   subject to   A_ub x <= b_ub,   A_eq x = b_eq,   x >= 0
 * with n variables, m_ub inequality rows and m_eq equality rows.  Every LP is assembled on the device into the tableau
 * `tableauModel` builds for the equivalent model (reference src/tableau.ts:47-137; width n + 1, height 1 + m_ub + 2 m_eq:
 * row 0 = +0.0, sign * c; then b_ub[i], A_ub[i, :]; then per equality b_eq[k], A_eq[k, :] and the row of their negations),
 * solved by `simplex(tableau, options)` (src/simplex.ts:106-144), one workgroup per LP, and read out on the device as
 * `solution()` reads it (src/YALPS.ts:8-50) into dense rows.  Values are taken as they lie in memory, NaN and infinities
 * included.  Per call one int32 per LP crosses PCIe: the statuses the host needs to decide about a rerun.
 *
 * An operand is (device pointer, element strides): element (i, r, c) of a matrix operand at ptr[i * batch + r * row + c * col],
 * element (i, r) of a vector operand at ptr[i * batch + r * row] (its col stride is ignored).  Strides are counted in
 * doubles and are >= 0; batch = 0 shares one operand among all LPs of the call; any row / col stride is legal (transposed
 * and sliced views); col = 1 is the fast case, read coalesced.
 *
 * Return protocol as yalps_hip.h: the YALPS_* codes below, negative = native failure with text through
 * yalps_lpdense_last_error() (per thread).  There is NO CPU fallback: without a usable gfx950 device
 * yalps_lpdense_create fails with YALPS_E_DEVICE.  A handle belongs to one thread at a time; its device buffers are
 * kept and grown between calls.
 *
 * Pointers and streams belong to the HIP runtime that made them.  A process that holds two HIP runtimes (a framework
 * that brings its own, loaded after this library) must hand over only what THIS library's runtime knows:
 * yalps_lpdense_solve asks it about every operand and output pointer and refuses what it does not know.
 *
 * Bounds (yalps_lpdense_solve_bounds).  lb, a vector operand of n elements per LP, means x >= lb and REPLACES x >= 0 for the
 * call (negative entries are legal; every entry is read); ub, read only at the n_upper variables upper_idx names (host memory,
 * ascending, shared by the call), means x[j] <= ub[j].  Either may be absent (a NULL descriptor).  The tableau as built, with
 * x = lb + x' substituted on the device:
 *   shift_sum(a, l) = sum of a[j] * l[j], every product rounded on its own, added in ONE order that depends on nothing but a
 *     and l: 64 partial sums p[k], each +0.0 plus the products of the columns j = k (mod 64) in ascending j; then
 *     p[k] += p[k + s] for k < s, s = 32, 16, 8, 4, 2, 1; the value is p[0].
 *   row 1 + i, column 0:  b_ub[i] - shift_sum(A_ub[i], lb); equality k: b_eq[k] - shift_sum(A_eq[k], lb) and, in the second row of
 *     the pair, its IEEE negation.  One subtraction; without lb none at all (not b - 0.0).  Coefficients, row 0 and cell (0, 0)
 *     are untouched.
 *   n_upper bound rows below the equality rows, in ascending variable index: column 0 = ub[j] - lb[j] (ub[j] without lb), 1.0 in
 *     the variable's column, +0.0 elsewhere: tableauModel's row of a constraint {"max": ...} in which variable j alone has a
 *     coefficient, 1.  Width n + 1, height 1 + m_ub + 2 m_eq + n_upper, which is what YALPS_LPDENSE_MAX_BYTES bounds.
 *   read-out: x = x' + lb, one addition per element whatever the status (NaN stays NaN, +inf stays +inf);
 *     objective = objective' + shift_sum(c, lb) with the caller's c, one addition after the rounding.
 *
 * Free variables (yalps_lpdense_solve_free).  The n_free variables free_idx names (host memory, ascending, shared by the call) have
 * no lower bound.  Freeness is host data and is not inferred on the device: at a variable free_idx does not name, an lb entry
 * of -inf is taken as it lies in memory, like every other value.  A free variable j is split as x[j] = p[j] - q[j] with p, q >= 0, built on the device:
 *   p keeps column 1 + j; the twins q are n_free generated columns behind the n originals in ascending j, column 1 + n + t for
 *     free_idx[t].  Width 1 + n + n_free, height as above, and YALPS_LPDENSE_MAX_BYTES bounds 8 * width * height.
 *   a twin cell is the IEEE negation of the cell of column 1 + j in the same row, in every operand row, as `m[...] = -coef` makes
 *     it: row 0 holds -(sign * c[j]), a zero becomes -0.0, the negated row of an equality holds A_eq[k, j] again.  It is a negation
 *     of the value read, not a second product.
 *   in the bound row of a free variable that upper_idx also lists the twin cell is -1.0, in every other bound row +0.0: x <= ub
 *     with no lower bound.
 *   lb is NOT read at a free variable: the effective lower bound l_eff[j] is +0.0 there and lb[j] elsewhere.  The product
 *     a[j] * (+0.0) is still formed and added in shift_sum (a non-finite coefficient gives NaN there), which runs over the n
 *     original columns only, in its one order; twins take no part in it.  A bound row of a free variable holds ub[j] - (+0.0) with
 *     lb given and ub[j] without.  Permutations are the identity over width + height; the padding columns of the pitch are +0.0.
 *   read-out: optimal: x[j] = v(p) - v(q), v the rule of x_out for each column on its own (basic and above precision: the value
 *     rounded to precision, else +0.0), one subtraction, then + l_eff[j] where lb is given; unbounded: +inf at the unbounded
 *     column, so x[free_idx[t]] = 0.0 - inf = -inf where that column is a twin; infeasible / cycled: NaN.
 *     objective = -sign * result + shift_sum(c, l_eff).
 *   marginals: ineqlin, eqlin and upper are unchanged (rows; pos[w + r] with the new width w).  For a free variable
 *     reduced[j] = s * (cost_nb(1 + j) - cost_nb(1 + n + t)) + 0.0 with cost_nb(v) = cost(pos[v]) where pos[v] < w, else 0: the full
 *     signed reduced cost, about 0 at an optimum, so that reduced = c - A_ub^T ineqlin - A_eq^T eqlin - scatter(upper) holds at
 *     every j.  Other variables keep their formula.
 * For finite data an LP is solve() of the equivalent model: the bounded call's model in x', plus one variable q<j> per free
 * variable behind all x<j>, in ascending j, listing the negated coefficient of every constraint x<j> lists, and -c[j].
 * Per-LP sets of free variables are out of scope.
 */
#ifndef YALPS_LPDENSE_H
#define YALPS_LPDENSE_H

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

#define YALPS_LPDENSE_MAX_BYTES (4 << 20) /* the largest tableau, 8 * (n + 1) * (1 + m_ub + 2 * m_eq) bytes */

typedef struct yalps_lpdense yalps_lpdense;

typedef struct yalps_lpdense_operand {
    const double *ptr; /* device memory; NULL where the operand has no element */
    int64_t batch, row, col;
} yalps_lpdense_operand;

const char *yalps_lpdense_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream.  The device's
 * default stream, whose handle is NULL, is named by hipStreamLegacy ((hipStream_t)1). */
int32_t yalps_lpdense_create(int32_t device, void *hip_stream, yalps_lpdense **out);
void yalps_lpdense_destroy(yalps_lpdense *d);

/* Host only (no device needed, no pointer dereferenced): what yalps_lpdense_solve checks of the shape and the operands
 * before it touches the device.  0, or YALPS_E_ARG with the reason in the error text: count < 0, a negative dimension, a
 * tableau above YALPS_LPDENSE_MAX_BYTES, an operand descriptor that is NULL, a negative stride, a NULL pointer of an
 * operand that has elements (count > 0 and: n > 0 for c; m_ub > 0 for b_ub, and n > 0 too for A_ub; likewise *_eq). */
int32_t yalps_lpdense_validate(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c,
                               const yalps_lpdense_operand *A_ub, const yalps_lpdense_operand *b_ub,
                               const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq);

/* yalps_lpdense_validate with the bounds of yalps_lpdense_solve_bounds, host only: the size limit with the height that counts
 * the n_upper bound rows, a negative stride of lb / ub (NULL descriptor: absent), a NULL pointer of one that has elements,
 * n_upper > 0 without ub, an index of upper_idx (host memory) outside 0 .. n-1 or not ascending. */
int32_t yalps_lpdense_validate_bounds(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c,
                                      const yalps_lpdense_operand *A_ub, const yalps_lpdense_operand *b_ub,
                                      const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq,
                                      const yalps_lpdense_operand *lb, const yalps_lpdense_operand *ub, int32_t n_upper,
                                      const int32_t *upper_idx);

/* yalps_lpdense_validate_bounds with the free variables of yalps_lpdense_solve_free, host only: the size limit with the width
 * that counts the n_free twin columns, n_free < 0, a NULL free_idx with n_free > 0, an index of free_idx (host memory) outside
 * 0 .. n-1 or not ascending. */
int32_t yalps_lpdense_validate_free(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c,
                                    const yalps_lpdense_operand *A_ub, const yalps_lpdense_operand *b_ub,
                                    const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq,
                                    const yalps_lpdense_operand *lb, const yalps_lpdense_operand *ub, int32_t n_upper,
                                    const int32_t *upper_idx, int32_t n_free, const int32_t *free_idx);

/* Solves LPs 0 .. count-1.  maximize != 0: maximise c . x, else minimise.  precision / maxPivots (may be +Infinity) /
 * checkCycles hold for the whole call.  keep_tableaux != 0 also keeps every final matrix on the device for
 * yalps_lpdense_tableau.  All four outputs are DEVICE pointers, contiguous, and may be NULL:
 *   x_out[count][n]       optimal: the variables' values, those above precision rounded to it, the others (a NaN too) +0.0;
 *                         unbounded: +0.0 but +inf at the unbounded variable (where it is one of the n); else NaN
 *   objective_out[count]  optimal: -sign * result; unbounded: sign * inf; else NaN       (sign = +1 maximise, -1 minimise)
 *   status_out[count]     int32, YALPS_OPTIMAL .. YALPS_CYCLED
 *   pivots_out[count]     int64
 * They are complete when the call returns.  gpu_ms_out (host, optional) = HIP-event time of the kernels.
 * count == 0 succeeds and launches nothing.  Before anything is enqueued every non-NULL operand and output pointer is
 * looked up in this library's HIP runtime (hipPointerGetAttributes): host memory, memory of another device and a pointer
 * the runtime does not know are refused with YALPS_E_ARG and a text that names the argument.  Returns 0 or a negative
 * error; nothing is launched when an argument is refused. */
int32_t yalps_lpdense_solve(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                            const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                            const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                            const yalps_lpdense_operand *b_eq, int32_t maximize, double precision, double maxPivots,
                            int32_t checkCycles, int32_t keep_tableaux, double *x_out, double *objective_out,
                            int32_t *status_out, int64_t *pivots_out, float *gpu_ms_out);

/* yalps_lpdense_solve (which is this call with three NULLs) plus the marginals of every LP, written by the workgroup that
 * solved it from the final row 0 and positionOfVariable: three more DEVICE pointers, contiguous, each may be NULL, looked up
 * and refused like the other outputs; one that has no element (m_ub = 0, m_eq = 0, n = 0 or count = 0) is never looked up
 * or written.  With s = +1 maximise, -1 minimise, w = n + 1, pos = the final positionOfVariable,
 * cost(c) = row0[c] < 0 ? row0[c] : 0 (a NaN row0[c] gives NaN), and for tableau row r
 * y(r) = -cost(pos[w + r]) where pos[w + r] < w (the row's slack is non-basic), else 0:
 *   ineqlin_out[count][m_ub]  optimal: s * y(1 + i) + 0.0; else NaN
 *   eqlin_out[count][m_eq]    optimal: s * (y(1 + m_ub + 2k) - y(2 + m_ub + 2k)) + 0.0 -- the row of b_eq[k] minus the row of
 *                             its negation; both slacks can be non-basic at once; else NaN
 *   reduced_out[count][n]     optimal: s * cost(pos[j + 1]) + 0.0 where pos[j + 1] < w (variable j is non-basic), else +0.0;
 *                             not optimal: NaN
 * (+ 0.0: a -0.0 becomes +0.0.)  "unbounded" gives NaN too: there is no dual solution.  These are d(objective_out) / d(b_ub),
 * d(objective_out) / d(b_eq) and the reduced costs of x >= 0 in the caller's own direction: for minimise scipy's
 * ineqlin.marginals, eqlin.marginals and lower.marginals, for maximise the negations of what scipy reports for -c; at a
 * degenerate vertex those of the basis the reference's pivot rule ends in.  For every optimal LP
 * objective = ineqlin . b_ub + eqlin . b_eq and reduced = c - A_ub^T ineqlin - A_eq^T eqlin, up to rounding.  They are what
 * yalps_amd.sensitivity gives as `dual` and `reduced_cost` for the equivalent model, bit for bit. */
int32_t yalps_lpdense_solve_duals(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                  const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                                  const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                                  const yalps_lpdense_operand *b_eq, int32_t maximize, double precision, double maxPivots,
                                  int32_t checkCycles, int32_t keep_tableaux, double *x_out, double *objective_out,
                                  int32_t *status_out, int64_t *pivots_out, double *ineqlin_out, double *eqlin_out,
                                  double *reduced_out, float *gpu_ms_out);

/* yalps_lpdense_solve_duals (which is this call with lb, ub and upper_out NULL and n_upper 0, and writes the bits it wrote
 * before) with bounds; see "Bounds" at the top for the tableau and the read-out.  lb / ub: operand descriptors or NULL;
 * upper_idx: HOST memory, n_upper ascending indices (copied before the call returns); lb, ub and upper_out are DEVICE pointers,
 * looked up and refused by name like the others.  With either descriptor given the call runs lp_dense_bounds_kernel
 * (libyalps_lpdense_bounds.so, which this library links); with neither, the boundless kernels.
 *   upper_out[count][n_upper]  optimal: s * y(1 + m_ub + 2 m_eq + t) + 0.0, ineqlin's formula on bound row t; else NaN
 * reduced_out is then the marginal of x >= lb (scipy's lower.marginals), upper_out that of x <= ub (upper.marginals).  For
 * every optimal LP, up to rounding, reduced = c - A_ub^T ineqlin - A_eq^T eqlin - scatter(upper) and
 * objective = ineqlin . b_ub + eqlin . b_eq + upper . ub + reduced . lb.  yalps_lpdense_solution and yalps_lpdense_tableau give
 * the taller tableau: height 1 + m_ub + 2 m_eq + n_upper. */
int32_t yalps_lpdense_solve_bounds(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                   const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                                   const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                                   const yalps_lpdense_operand *b_eq, const yalps_lpdense_operand *lb,
                                   const yalps_lpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx, int32_t maximize,
                                   double precision, double maxPivots, int32_t checkCycles, int32_t keep_tableaux, double *x_out,
                                   double *objective_out, int32_t *status_out, int64_t *pivots_out, double *ineqlin_out,
                                   double *eqlin_out, double *reduced_out, double *upper_out, float *gpu_ms_out);

/* yalps_lpdense_solve_bounds (which is this call with n_free = 0, and writes the bits it wrote before) with free variables; see
 * "Free variables" at the top.  free_idx: HOST memory, n_free ascending indices (copied before the call returns).  With
 * n_free > 0 the call runs lp_dense_free_kernel (libyalps_lpdense_free.so, which this library links), with or without lb / ub
 * (NULL descriptors: absent).  x_out and reduced_out stay [count][n]; yalps_lpdense_solution and yalps_lpdense_tableau give the
 * wider tableau: width 1 + n + n_free. */
int32_t yalps_lpdense_solve_free(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                 const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                                 const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                                 const yalps_lpdense_operand *b_eq, const yalps_lpdense_operand *lb,
                                 const yalps_lpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx, int32_t n_free,
                                 const int32_t *free_idx, int32_t maximize, double precision, double maxPivots, int32_t checkCycles,
                                 int32_t keep_tableaux, double *x_out, double *objective_out, int32_t *status_out, int64_t *pivots_out,
                                 double *ineqlin_out, double *eqlin_out, double *reduced_out, double *upper_out, float *gpu_ms_out);

/* LP i of the last solve, copied to the HOST (for tests and debugging): what solution() reads -- column 0 (height
 * doubles) and both permutations (width + height int32 each).  NULL pointers are skipped. */
int32_t yalps_lpdense_solution(yalps_lpdense *d, int32_t i, double *col0, int32_t *positionOfVariable,
                               int32_t *variableAtPosition);
/* LP i of the last solve: the whole final matrix, row-major width * height, to the host.  Needs keep_tableaux. */
int32_t yalps_lpdense_tableau(yalps_lpdense *d, int32_t i, double *matrix);
/* Text about the last solve: launches made, per launch the kernel's spelling, its size class, LP count, grid and LDS
 * bytes, and the LPs rerun because their checkCycles history overflowed.  Writes at most len - 1 characters and returns the
 * length of the whole text: a return value >= len means the text was cut (call again with a larger buffer). */
int32_t yalps_lpdense_info(const yalps_lpdense *d, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_LPDENSE_H */
