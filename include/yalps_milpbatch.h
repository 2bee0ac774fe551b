/*
 * yalps_milpbatch.h -- C ABI of libyalps_milpbatch.so: many independent small MILPs in one call (MI355X, gfx950).
 *
 * yalps_hip.h's yalps_milp_f64 runs ONE branch-and-cut tree per call and waits for the device once per node batch.  Here
 * `count` unrelated models with integer variables advance together: a root pass solves every root LP (one workgroup per
 * root, the kernels of yalps_lpbatch.h) and keeps the optimal tableaux on the device; then, round by round, the nodes that
 * the trees want next -- of any mix of roots and shapes -- are evaluated in shared launches (one workgroup per node,
 * milp_node_kernel: applyCuts next to the resident root, reference src/branchAndCut.ts:22-61, then simplex()) with one wait
 * per round.  Every tree follows the reference's search (src/branchAndCut.ts:89-176) exactly as yalps_milp_f64 does:
 * nodes are committed in the reference's pop order, and evaluating a node ahead of its turn changes nothing.
 *
 * Three levels: the root pass and the node pass on their own (yalps_milpbatch_roots / _nodes), the whole solve
 * (yalps_milpbatch_solve), and the same lockstep driver without a device, its node evaluator a callback
 * (yalps_milpbatch_search).
 *
 * Return protocol as yalps_hip.h: the YALPS_* codes below, negative = native failure with text through
 * yalps_milpbatch_last_error() (per thread).  There is NO CPU fallback: without a usable gfx950 device
 * yalps_milpbatch_create fails with YALPS_E_DEVICE.  A handle belongs to one thread at a time; its device buffers are
 * kept and grown between calls.
 *
 * Models are given as yalps_lpbatch.h gives LPs: the cells `tableauModel` writes (row, col, val sorted by (row, col),
 * strictly increasing).  Size limit: a node's tableau, 8 * width * (height + cuts) bytes, may not exceed
 * YALPS_MILPBATCH_MAX_BYTES; a model's largest possible node has 2 * n_integers cuts.
 */
#ifndef YALPS_MILPBATCH_H
#define YALPS_MILPBATCH_H

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
#define YALPS_MILPBATCH_TIMEDOUT 4 /* status of a model whose search ended unfinished (src/branchAndCut.ts:166-173) */

#define YALPS_MILPBATCH_MAX_BYTES (4 << 20)

typedef struct yalps_milpbatch yalps_milpbatch;

const char *yalps_milpbatch_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream. */
int32_t yalps_milpbatch_create(int32_t device, void *hip_stream, yalps_milpbatch **out);
void yalps_milpbatch_destroy(yalps_milpbatch *b);

/* ---- low level: the root pass ----
 * Solves roots 0 .. count-1 (arguments as yalps_lpbatch_solve) and keeps every final tableau and both permutations on
 * the device for yalps_milpbatch_nodes.  status / result / pivots are per root and may be NULL. */
int32_t yalps_milpbatch_roots(yalps_milpbatch *b, int32_t count, const int32_t *width, const int32_t *height,
                              const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                              const double *precision, const double *maxPivots, const int32_t *checkCycles,
                              int32_t *status_out, double *result_out, int64_t *pivots_out);
/* Root i of the last root pass: column 0 (height doubles), both permutations (width + height int32 each), and, where
 * `matrix` is not NULL, the whole final matrix (row-major width * height). */
int32_t yalps_milpbatch_root(yalps_milpbatch *b, int32_t i, double *col0, int32_t *positionOfVariable,
                             int32_t *variableAtPosition, double *matrix);

/* ---- low level: the node pass ----
 * Nodes 0 .. count-1 in shared launches, one per (size class, checkCycles) pair, and one wait.  Node k is root
 * root_index[k] of the last root pass plus the cuts [cut_offsets[k], cut_offsets[k + 1]) of cut_sign (+1: x <= value,
 * -1: x >= value) / cut_var (1 .. width - 1 of its root) / cut_val.  It is solved with its root's precision, maxPivots
 * and checkCycles; maxPivots_override (NULL: each root's own) gives every node its own budget instead -- a budget of 0
 * returns the node's INITIAL tableau with status YALPS_CYCLED.  keep_tableaux != 0 also keeps every final matrix for
 * yalps_milpbatch_node_tableau.  status / result / pivots / height (root height + cuts) are per node and may be NULL.
 * Refused with YALPS_E_ARG and the node's index in the error text, before any device call: a root index out of range,
 * cut offsets that decrease, a cut on a variable out of range, a node above YALPS_MILPBATCH_MAX_BYTES. */
int32_t yalps_milpbatch_nodes(yalps_milpbatch *b, int32_t count, const int32_t *root_index, const int64_t *cut_offsets,
                              const int32_t *cut_sign, const int32_t *cut_var, const double *cut_val,
                              const double *maxPivots_override, int32_t keep_tableaux, int32_t *status_out,
                              double *result_out, int64_t *pivots_out, int32_t *height_out);
/* Host only: the argument checks of yalps_milpbatch_nodes against roots of the given shapes. */
int32_t yalps_milpbatch_validate_nodes(int32_t n_roots, const int32_t *root_width, const int32_t *root_height,
                                       int32_t count, const int32_t *root_index, const int64_t *cut_offsets,
                                       const int32_t *cut_var);
/* Node k of the last node pass: column 0 (its height doubles) and both permutations (width + height int32 each). */
int32_t yalps_milpbatch_node(yalps_milpbatch *b, int32_t k, double *col0, int32_t *positionOfVariable,
                             int32_t *variableAtPosition);
/* Node k of the last node pass: the whole final matrix, row-major width * height.  Needs keep_tableaux. */
int32_t yalps_milpbatch_node_tableau(yalps_milpbatch *b, int32_t k, double *matrix);

/* ---- the whole solve ----
 * Models 0 .. count-1: cells as in the root pass; the integer variables of model i (indices 1 .. width - 1) are
 * integers[int_offsets[i] .. int_offsets[i + 1]); sign is the model's objective sign (+1 maximise, -1 minimise, as
 * tableauModel returns it); precision / maxPivots / checkCycles / tolerance / timeout (milliseconds, may be +Infinity)
 * / maxIterations are the reference's Options, per model.  node_batch >= 1: per round a tree asks for the node it popped
 * plus its next-best node_batch - 1 frontier nodes.
 * Per model: status (YALPS_* or YALPS_MILPBATCH_TIMEDOUT), result (NaN without a solution), and stats[2 * i] = nodes
 * used (consumed in pop order), stats[2 * i + 1] = nodes evaluated.  call_stats (optional): [0] rounds, [1] launches
 * (root pass included), [2] HIP-event microseconds of all kernels.  The best tableau of each model is read with
 * yalps_milpbatch_solution. */
int32_t yalps_milpbatch_solve(yalps_milpbatch *b, int32_t count, const int32_t *width, const int32_t *height,
                              const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                              const int64_t *int_offsets, const int32_t *integers, const double *sign,
                              const double *precision, const double *maxPivots, const int32_t *checkCycles,
                              const double *tolerance, const double *timeout_ms, const double *maxIterations,
                              int32_t node_batch, int32_t *status_out, double *result_out, int64_t *stats_out,
                              int64_t *call_stats_out);
/* Host only: what yalps_milpbatch_solve checks of the integers and the node sizes before it touches the device. */
int32_t yalps_milpbatch_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *int_offsets,
                                 const int32_t *integers, int32_t node_batch);
/* Model i of the last solve, what solution() reads of its best tableau (src/YALPS.ts:18-19,32): *height_out rows,
 * column 0 (room for height + 2 * n_integers doubles) and both permutations (room for width + height + 2 * n_integers). */
int32_t yalps_milpbatch_solution(yalps_milpbatch *b, int32_t i, int32_t *height_out, double *col0,
                                 int32_t *positionOfVariable, int32_t *variableAtPosition);

/* ---- host only: the lockstep driver with the node evaluator as a callback (no device, no handle) ----
 * eval evaluates `count` nodes: node k belongs to model model[k] and has the cuts [cut_offsets[k], cut_offsets[k + 1]).
 * It fills status[k], result[k], height[k], and -- packed node after node, node k's height doubles / width + height int32
 * following node k - 1's -- column 0 and both permutations of each solved node.  A negative return value ends the search
 * with that code.  consumed (optional) is called once per node a tree consumes, in that tree's pop order. */
typedef int32_t (*yalps_milpbatch_eval_fn)(void *user, int32_t count, const int32_t *model, const int64_t *cut_offsets,
                                           const int32_t *cut_sign, const int32_t *cut_var, const double *cut_val,
                                           int32_t *status, double *result, int32_t *height, double *col0, int32_t *pos,
                                           int32_t *var);
typedef void (*yalps_milpbatch_consumed_fn)(void *user, int32_t model, double eval, int32_t n_cuts, const int32_t *cut_sign,
                                            const int32_t *cut_var, const double *cut_val);
/* Roots are given solved: status, result, and packed model after model column 0 (height doubles) and both permutations
 * (width + height int32).  Outputs per model as yalps_milpbatch_solve's; the best tableaux come back packed with room for
 * height + 2 * n_integers rows per model (column 0) and width + height + 2 * n_integers entries (permutations).
 * rounds_out (optional): the number of eval calls. */
int32_t yalps_milpbatch_search(int32_t count, const int32_t *width, const int32_t *height, const int32_t *root_status,
                               const double *root_result, const double *root_col0, const int32_t *root_pos,
                               const int32_t *root_var, const int64_t *int_offsets, const int32_t *integers,
                               const double *sign, const double *precision, const double *tolerance,
                               const double *timeout_ms, const double *maxIterations, int32_t node_batch,
                               yalps_milpbatch_eval_fn eval, yalps_milpbatch_consumed_fn consumed, void *user,
                               int32_t *status_out, double *result_out, int32_t *height_out, double *col0_out,
                               int32_t *pos_out, int32_t *var_out, int64_t *stats_out, int64_t *rounds_out);

/* Text about the last root pass / node pass / solve: "rounds=.. launches=.. reruns=.. rerun_nodes=[..] gpu_us=..", then
 * one line per launch with the kernel's spelling, its size class, node (or LP) count, grid and LDS bytes.  Writes at most
 * len - 1 characters and returns the length of the whole text (>= len: cut, call again with a larger buffer). */
int32_t yalps_milpbatch_info(const yalps_milpbatch *b, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_MILPBATCH_H */
