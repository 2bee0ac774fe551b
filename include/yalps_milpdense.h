/*
 * yalps_milpdense.h -- C ABI of libyalps_milpdense.so: a batch of dense MILPs of one shape, read from and answered in DEVICE
 * memory, every branch-and-cut tree walked on the device (MI355X, gfx950).
 *
 * yalps_lpdense.h reads dense LPs where they lie; yalps_milptree.h walks whole trees on the device but takes packed cell
 * lists from host memory.  Here the `count` MILPs of a call share one shape and one set of integer and binary variables and
 * lie in device memory as yalps_lpdense.h's operands:
 *     maximize | minimize  c . x   subject to   A_ub x <= b_ub,   A_eq x = b_eq,   x >= 0,
 *     x[j] integer for j in `integers`,   x[j] in {0, 1} for j in `binaries`
 * Three device parts on one stream:
 *   root pass   milp_dense_root_kernel assembles the tableau `tableauModel` builds for the equivalent model (reference
 *               src/tableau.ts:47-137): the 1 + m_ub + 2 m_eq rows of yalps_lpdense.h, then one row per binary variable in
 *               ascending index -- column 0 1.0, the variable's column 1.0, the rest +0.0 -- so width = n + 1 and
 *               height = 1 + m_ub + 2 m_eq + n_binaries; `simplex` solves it, one workgroup per MILP, tableaux kept.
 *   tree pass   milp_tree_kernel as yalps_milptree.h runs it (src/branchAndCut.ts:89-176): arenas, reruns with four times
 *               the room, and above the cap the status YALPS_MILPDENSE_OVERFLOW.  Skipped when n_integers = 0, as solve()
 *               never enters branchAndCut then (src/YALPS.ts:81).
 *   epilogue    milp_dense_solution_kernel reads every best tableau as `solution()` does (src/YALPS.ts:8-50) into dense rows.
 * Values are taken as they lie in memory, NaN and infinities included.  The device reads no clock: the timeout is +Infinity.
 *
 * Variable bounds (yalps_milpdense_solve_bounds): lb <= x replaces x >= 0 and x[j] <= ub[j] for the n_upper listed variables,
 * as yalps_lpdense_solve_bounds has them, with three rules that come from the variables being integer -- all three decided
 * from the host lists, none costs the device anything:
 *   1. the effective lower bound l_eff[j] is lb[j] at a continuous variable, ceil(lb[j]) at an integer one (IEEE ceil: -0.5
 *      gives -0.0, NaN and the infinities pass through) and +0.0 at a binary one, where lb is not read.  x = l_eff + x' keeps
 *      "x' integral <=> x integral": the tree pass branches on x' and knows nothing of bounds.  Everything
 *      yalps_lpdense_solve_bounds does with lb is done with l_eff: every right-hand side is moved by shift_sum(row, l_eff) in
 *      yalps_lpdense.h's order of summation (the product with +0.0 at a binary column is still formed), a bound row holds
 *      ub[j] - l_eff[j], x = x' + l_eff, objective = objective' + shift_sum(c, l_eff).
 *   2. a binary variable has no bound row of its own: ub is not read there, and upper_idx may not name one.
 *   3. rows: yalps_lpdense.h's, then the n_upper bound rows in ascending index, then the binary rows; width n + 1, height
 *      1 + m_ub + 2 m_eq + n_upper + n_binaries, and the largest node counts them.
 * The root pass and the epilogue of such a call are milp_dense_bounds_root_kernel and milp_dense_bounds_solution_kernel, the
 * code object of libyalps_milpdense_bounds.so, which this library links; a call without bounds launches the kernels, and
 * returns the bits, it always did.  There are no duals: a node's duals are not the model's.
 * Per call the descriptors go up (one call description, the integer lists, 72 + 80 bytes per tree) and one int32 per tree
 * per pass comes back: the statuses the host needs to decide about a rerun.
 *
 * Operands, strides, the return protocol, the stream rule and the pointer rule are yalps_lpdense.h's: element (i, r, c) of a
 * matrix operand at ptr[i * batch + r * row + c * col]; negative = native failure with text through
 * yalps_milpdense_last_error() (per thread); NO CPU fallback; every operand and output pointer is looked up in this
 * library's HIP runtime and refused by name when it is host memory, memory of another device, or unknown to it.
 *
 * Environment (test hooks, read by yalps_milpdense_create): YALPS_MILPDENSE_ARENA (heap entries of the first arena, default
 * 128), YALPS_MILPDENSE_ARENA_MAX (the cap, default 65536), YALPS_MILPDENSE_HIST (first checkCycles history capacity of both
 * passes) and YALPS_MILPDENSE_GRID (workgroups per tree launch: one workgroup then walks many trees one after the other).
 */
#ifndef YALPS_MILPDENSE_H
#define YALPS_MILPDENSE_H

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
#define YALPS_MILPDENSE_TIMEDOUT 4 /* the search ended unfinished (src/branchAndCut.ts:166-173) */
#define YALPS_MILPDENSE_OVERFLOW 5 /* the tree's frontier outgrew the largest arena: no result */

#define YALPS_MILPDENSE_MAX_BYTES (4 << 20) /* the largest node, 8 * (n + 1) * (height + 2 * n_integers) bytes */

typedef struct yalps_milpdense yalps_milpdense;

typedef struct yalps_milpdense_operand {
    const double *ptr; /* device memory; NULL where the operand has no element */
    int64_t batch, row, col;
} yalps_milpdense_operand;

const char *yalps_milpdense_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream.  The device's
 * default stream, whose handle is NULL, is named by hipStreamLegacy ((hipStream_t)1). */
int32_t yalps_milpdense_create(int32_t device, void *hip_stream, yalps_milpdense **out);
void yalps_milpdense_destroy(yalps_milpdense *d);

/* Host only (no device needed, no pointer dereferenced): what yalps_milpdense_solve checks before it touches the device.
 * 0, or YALPS_E_ARG with the reason in the error text: everything yalps_lpdense_validate refuses, by the same words; a
 * negative n_integers or n_binaries; a NULL list that has elements; `integers` or `binaries` (HOST arrays of 0-based
 * variable indices) not strictly ascending or out of 0 .. n - 1; a binary variable that is not in `integers` (the integer
 * list is the union of both sets); a largest node of 8 * (n + 1) * (height + 2 * n_integers) bytes above
 * YALPS_MILPDENSE_MAX_BYTES. */
int32_t yalps_milpdense_validate(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c,
                                 const yalps_milpdense_operand *A_ub, const yalps_milpdense_operand *b_ub,
                                 const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq,
                                 int32_t n_integers, const int32_t *integers, int32_t n_binaries, const int32_t *binaries);

/* Solves MILPs 0 .. count-1.  maximize != 0: maximise c . x, else minimise.  precision / maxPivots (may be +Infinity) /
 * checkCycles / tolerance / maxIterations are the reference's Options, for the whole call.  trace_cap >= 0: the first
 * trace_cap nodes every tree consumes are recorded for yalps_milpdense_trace.  All six outputs are DEVICE pointers,
 * contiguous, and may be NULL:
 *   x_out[count][n]         optimal, or timedout with a result: the variables' values in the best tableau, those above
 *                           precision rounded to it, the others (a NaN too) +0.0; unbounded: +0.0 but +inf at the unbounded
 *                           variable; else NaN
 *   objective_out[count]    optimal / timedout with a result: -sign * result; unbounded: sign * inf; else NaN
 *   status_out[count]       int32, YALPS_OPTIMAL .. YALPS_CYCLED, YALPS_MILPDENSE_TIMEDOUT or YALPS_MILPDENSE_OVERFLOW
 *   nodes_out[count]        int64, nodes consumed (0 without a tree pass, and for an overflowed tree)
 *   node_pivots_out[count]  int64, the sum of their pivots (likewise)
 *   root_pivots_out[count]  int64, the root LP's pivots
 * An overflowed tree has NaN in x_out and objective_out; yalps_milpdense_overflowed names those trees.  With n_integers = 0
 * the first three outputs and root_pivots_out are yalps_lpdense_solve's x, objective, status and pivots, bit for bit.
 * They are complete when the call returns.  call_stats_out (host, optional): [0] trees run again, [1] launches (all three
 * parts), [2] overflowed trees, [3] / [4] / [5] HIP-event microseconds of root pass, tree pass and epilogue.
 * count == 0 succeeds and launches nothing.  Nothing is launched when an argument is refused. */
int32_t yalps_milpdense_solve(yalps_milpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                              const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                              const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq,
                              const yalps_milpdense_operand *b_eq, int32_t n_integers, const int32_t *integers,
                              int32_t n_binaries, const int32_t *binaries, int32_t maximize, double precision,
                              double maxPivots, int32_t checkCycles, double tolerance, double maxIterations,
                              int32_t trace_cap, double *x_out, double *objective_out, int32_t *status_out,
                              int64_t *nodes_out, int64_t *node_pivots_out, int64_t *root_pivots_out,
                              int64_t *call_stats_out);

/* yalps_milpdense_validate with bounds: the height counts the n_upper bound rows, and on top of its refusals come
 * yalps_lpdense_validate_bounds', by the same words under this library's name -- a negative n_upper, a negative stride or a NULL
 * pointer of lb / ub where they have elements, n_upper > 0 without ub, a NULL upper_idx, upper_idx[t] outside 0 .. n-1 or not
 * ascending -- and "variable j is binary" for an upper_idx entry that is in `binaries`.  lb and ub may be NULL descriptors
 * (absent); upper_idx is a HOST list. */
int32_t yalps_milpdense_validate_bounds(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c,
                                        const yalps_milpdense_operand *A_ub, const yalps_milpdense_operand *b_ub,
                                        const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq,
                                        const yalps_milpdense_operand *lb, const yalps_milpdense_operand *ub, int32_t n_upper,
                                        const int32_t *upper_idx, int32_t n_integers, const int32_t *integers, int32_t n_binaries,
                                        const int32_t *binaries);

/* yalps_milpdense_solve with bounds (the rules above).  lb[count][n] and ub[count][n] are DEVICE operands read through
 * (batch, row) strides -- col unused; lb at every variable that is not binary, ub at upper_idx[0 .. n_upper) only -- and are
 * looked up and refused by name like the others.  With both descriptors NULL (and n_upper = 0) the call is
 * yalps_milpdense_solve.  With n_integers = 0 the first three outputs and root_pivots_out are yalps_lpdense_solve_bounds' x,
 * objective, status and pivots, bit for bit.  yalps_milpdense_solution / _trace speak of the tableau in x': heights count the
 * bound rows, column 0 is not moved back. */
int32_t yalps_milpdense_solve_bounds(yalps_milpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                     const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                                     const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq,
                                     const yalps_milpdense_operand *b_eq, const yalps_milpdense_operand *lb,
                                     const yalps_milpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx,
                                     int32_t n_integers, const int32_t *integers, int32_t n_binaries, const int32_t *binaries,
                                     int32_t maximize, double precision, double maxPivots, int32_t checkCycles, double tolerance,
                                     double maxIterations, int32_t trace_cap, double *x_out, double *objective_out,
                                     int32_t *status_out, int64_t *nodes_out, int64_t *node_pivots_out, int64_t *root_pivots_out,
                                     int64_t *call_stats_out);

/* Free variables.  free_idx is a HOST list of n_free 0-based indices, strictly ascending: the variables without a lower bound.
 * The rules, all decided on the host:
 *   1. the split is yalps_lpdense_solve_free's: x[j] = p[j] - q[j]; p keeps column 1 + j, the n_free twins q are generated
 *      columns behind the n originals in ascending j, each cell the IEEE negation of the cell written at column 1 + j of that
 *      row (one strided read, not a second product), -1.0 in the bound row of a free variable upper_idx lists, +0.0 in every
 *      other generated row, the binary rows included.  Width 1 + n + n_free.
 *   2. lb is not read at a free variable: l_eff[j] is +0.0 there, with no ceil, integer or not; the product with +0.0 is still
 *      formed and added in shift_sum, which runs over the n original columns only.  Elsewhere l_eff is the bounded call's.
 *   3. a binary variable cannot be free: an entry of free_idx that is in `binaries` is refused ("variable j is binary").
 *   4. a free integer variable has two integer columns: milp_tree_kernel is handed the n_integers columns 1 + j in ascending
 *      j, then the twin columns of the free integer variables in ascending j (the whole list ascends):
 *      n_int_eff = n_integers + |free & integers| columns, tree slices of height + 2 * n_int_eff rows, and a largest node of
 *      8 * (1 + n + n_free) * (height + 2 * n_int_eff) bytes, which is what YALPS_MILPDENSE_MAX_BYTES bounds and the refusal
 *      says.
 *   5. rows: yalps_lpdense's, then the n_upper bound rows, then the binary rows, as with bounds.
 *   6. x_out[j] of a free variable, from the best tableau: optimal / timedout with a result v(p) - v(q), each v the rule above
 *      on its own column, one subtraction, then + l_eff[j] where lb is given; unbounded: +inf at the unbounded column, so -inf
 *      where that column is a twin; else NaN.  objective_out = objective' + shift_sum(c, l_eff), one addition.
 * yalps_milpdense_validate_free: yalps_milpdense_validate_bounds' refusals with that width and that largest node, plus a
 * negative n_free, a NULL free_idx, and free_idx out of 0 .. n - 1, not strictly ascending, or naming a binary variable. */
int32_t yalps_milpdense_validate_free(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c,
                                      const yalps_milpdense_operand *A_ub, const yalps_milpdense_operand *b_ub,
                                      const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq,
                                      const yalps_milpdense_operand *lb, const yalps_milpdense_operand *ub, int32_t n_upper,
                                      const int32_t *upper_idx, int32_t n_free, const int32_t *free_idx, int32_t n_integers,
                                      const int32_t *integers, int32_t n_binaries, const int32_t *binaries);

/* yalps_milpdense_solve_bounds with free variables (the rules above); lb and ub may both be NULL.  With n_free = 0 the call is
 * yalps_milpdense_solve_bounds (or, with neither descriptor, yalps_milpdense_solve): the same kernels, the same bits.  With
 * n_free > 0 it runs milp_dense_free_root_kernel and milp_dense_free_solution_kernel.  With n_integers = 0 the first three
 * outputs and root_pivots_out are yalps_lpdense_solve_free's x, objective, status and pivots, bit for bit.
 * yalps_milpdense_solution / _trace speak of the split tableau: width 1 + n + n_free, cut variables may be twin columns, and
 * "n_integers" in their room rules reads n_int_eff. */
int32_t yalps_milpdense_solve_free(yalps_milpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                   const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                                   const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq,
                                   const yalps_milpdense_operand *b_eq, const yalps_milpdense_operand *lb,
                                   const yalps_milpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx, int32_t n_free,
                                   const int32_t *free_idx, int32_t n_integers, const int32_t *integers, int32_t n_binaries,
                                   const int32_t *binaries, int32_t maximize, double precision, double maxPivots, int32_t checkCycles,
                                   double tolerance, double maxIterations, int32_t trace_cap, double *x_out, double *objective_out,
                                   int32_t *status_out, int64_t *nodes_out, int64_t *node_pivots_out, int64_t *root_pivots_out,
                                   int64_t *call_stats_out);

/* The trees of the last solve that ended YALPS_MILPDENSE_OVERFLOW, ascending: at most `cap` indices into ids (HOST, may be
 * NULL with cap = 0).  Returns their number. */
int32_t yalps_milpdense_overflowed(const yalps_milpdense *d, int32_t *ids, int32_t cap);

/* MILP i of the last solve, copied to the HOST (for tests and debugging): the tree's status and result, and what solution()
 * reads of its best tableau -- *height_out rows, column 0 (room for height + 2 * n_integers doubles) and both permutations
 * (room for width + height + 2 * n_integers).  NULL pointers are skipped. */
int32_t yalps_milpdense_solution(yalps_milpdense *d, int32_t i, int32_t *status_out, double *result_out, int32_t *height_out,
                                 double *col0, int32_t *positionOfVariable, int32_t *variableAtPosition);
/* MILP i of the last solve (trace_cap > 0), as yalps_milptree_trace: its first *count_out <= trace_cap consumed nodes in pop
 * order, cuts packed node after node (room for trace_cap * 2 * n_integers each).  Any output may be NULL. */
int32_t yalps_milpdense_trace(yalps_milpdense *d, int32_t i, int32_t *count_out, double *eval, int32_t *status, double *result,
                              int64_t *pivots, int32_t *height, int32_t *cut_sign, int32_t *cut_var, double *cut_val);
/* Text about the last solve: "launches=.. reruns=.. overflows=.. gpu_us=.. root_us=.. tree_us=.. epilogue_us=..
 * rerun_lps=[..] rerun_trees=[..]", then one line per launch with the kernel's spelling, its size class, LP or tree count,
 * grid, LDS bytes, history and arena capacity.  Writes at most len - 1 characters and returns the length of the whole text
 * (>= len: cut, call again with a larger buffer). */
int32_t yalps_milpdense_info(const yalps_milpdense *d, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_MILPDENSE_H */
