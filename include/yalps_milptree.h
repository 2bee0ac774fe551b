/*
 * yalps_milptree.h -- C ABI of libyalps_milptree.so: many independent small MILPs, every branch-and-cut tree walked on the
 * device (MI355X, gfx950).
 *
 * yalps_milpbatch.h advances its trees in rounds: the host pops, packs, launches milp_node_kernel, waits and reads back.
 * Here the search loop of the reference (src/branchAndCut.ts:89-176) runs inside the kernel.  A root pass solves every root
 * LP (the kernels of yalps_lpbatch.h, tableaux kept on the device); then milp_tree_kernel: one workgroup takes a tree from a
 * device counter and walks it to its end -- pop, applyCuts next to the resident root, simplex(), mostFractionalVar, push the
 * children, keep the incumbent -- and takes the next tree.  One launch per (size class, checkCycles) pair, no rounds.  Every
 * tree's node sequence, best tableau, status and result are the reference's, as yalps_milpbatch_solve gives them.
 *
 * The frontier of a tree lives in an arena of the workgroup (heap entries and cut lists); a tree that outgrows it, or a node
 * whose checkCycles history does, runs again alone from its root with four times the room.  Above a cap on the arena a tree
 * gets the status YALPS_MILPTREE_OVERFLOW and no result; the caller solves it another way (yalps_amd.solve.milptree_solve
 * sends it through yalps_milpbatch_solve).
 *
 * The device reads no clock: timeout_ms must be +Infinity, or <= 0 ("timed out before the first node").
 *
 * Return protocol as yalps_hip.h: the YALPS_* codes below, negative = native failure with text through
 * yalps_milptree_last_error() (per thread).  There is NO CPU fallback: without a usable gfx950 device
 * yalps_milptree_create fails with YALPS_E_DEVICE.  A handle belongs to one thread at a time.
 *
 * Environment (test hooks, read by yalps_milptree_create): YALPS_MILPTREE_ARENA (heap entries of the first arena, default
 * 128), YALPS_MILPTREE_ARENA_MAX (the cap, default 65536), YALPS_MILPTREE_ARENA_BYTES (bound on the arena buffer of a pass
 * that runs trees again, default 2 GiB: beyond it those trees get YALPS_MILPTREE_OVERFLOW too), YALPS_MILPTREE_HIST (first
 * checkCycles history capacity) and YALPS_MILPTREE_GRID (workgroups per launch: one workgroup then walks many trees one after
 * the other).
 */
#ifndef YALPS_MILPTREE_H
#define YALPS_MILPTREE_H

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
#define YALPS_MILPTREE_TIMEDOUT 4 /* the search ended unfinished (src/branchAndCut.ts:166-173) */
#define YALPS_MILPTREE_OVERFLOW 5 /* the tree's frontier outgrew the largest arena: no result */

#define YALPS_MILPTREE_MAX_BYTES (4 << 20)

typedef struct yalps_milptree yalps_milptree;

const char *yalps_milptree_last_error(void);

/* hip_stream: NULL = a private stream; otherwise every kernel / copy is enqueued on the caller's HIP stream. */
int32_t yalps_milptree_create(int32_t device, void *hip_stream, yalps_milptree **out);
void yalps_milptree_destroy(yalps_milptree *b);

/* Models 0 .. count-1 as yalps_milpbatch_solve takes them (cells of the root LP, integer variables, objective sign, the
 * reference's Options per model).  trace_cap >= 0: the first trace_cap nodes every tree consumes are recorded for
 * yalps_milptree_trace (0: no trace).  Per model: status (YALPS_*, YALPS_MILPTREE_TIMEDOUT or YALPS_MILPTREE_OVERFLOW),
 * result (NaN without a solution), stats[2 * i] = nodes consumed, stats[2 * i + 1] = the sum of their pivots.
 * call_stats (optional): [0] reruns, [1] launches (root pass included), [2] HIP-event microseconds of all kernels. */
int32_t yalps_milptree_solve(yalps_milptree *b, int32_t count, const int32_t *width, const int32_t *height,
                             const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                             const int64_t *int_offsets, const int32_t *integers, const double *sign,
                             const double *precision, const double *maxPivots, const int32_t *checkCycles,
                             const double *tolerance, const double *timeout_ms, const double *maxIterations,
                             int32_t trace_cap, int32_t *status_out, double *result_out, int64_t *stats_out,
                             int64_t *call_stats_out);
/* Host only: what yalps_milptree_solve checks of the integers, the node sizes and the timeouts before it touches the
 * device (timeout_ms may be NULL).  An error names the model. */
int32_t yalps_milptree_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *int_offsets,
                                const int32_t *integers, const double *timeout_ms);
/* Model i of the last solve, what solution() reads of its best tableau: *height_out rows, column 0 (room for
 * height + 2 * n_integers doubles) and both permutations (room for width + height + 2 * n_integers). */
int32_t yalps_milptree_solution(yalps_milptree *b, int32_t i, int32_t *height_out, double *col0,
                                int32_t *positionOfVariable, int32_t *variableAtPosition);
/* Model i of the last solve (trace_cap > 0): its first *count_out <= trace_cap consumed nodes in pop order.  Per node k:
 * eval[k], status[k], result[k], pivots[k], height[k] and its height[k] - root height cuts, packed node after node in
 * cut_sign / cut_var / cut_val (room for trace_cap * 2 * n_integers each).  Any output may be NULL. */
int32_t yalps_milptree_trace(yalps_milptree *b, int32_t i, int32_t *count_out, double *eval, int32_t *status, double *result,
                             int64_t *pivots, int32_t *height, int32_t *cut_sign, int32_t *cut_var, double *cut_val);

/* ---- host only: the same search rules with the node evaluator as a callback (no device, no handle) ----
 * Arguments as yalps_milpbatch_search without node_batch.  eval is called with one node at a time (count == 1): it fills
 * status[0], result[0], height[0] and column 0 and both permutations of the solved node.  A negative return value ends the
 * search with that code.  consumed (optional) sees every node of a finished tree, in pop order.
 * arena >= 2: heap entries of a tree's first arena; a tree that outgrows it runs again from its root with four times as
 * many, up to arena_max, above which its status is YALPS_MILPTREE_OVERFLOW.  stats[2 * i] = nodes consumed,
 * stats[2 * i + 1] = nodes evaluated (reruns included); reruns_out (optional): the number of reruns. */
typedef int32_t (*yalps_milptree_eval_fn)(void *user, int32_t count, const int32_t *model, const int64_t *cut_offsets,
                                          const int32_t *cut_sign, const int32_t *cut_var, const double *cut_val,
                                          int32_t *status, double *result, int32_t *height, double *col0, int32_t *pos,
                                          int32_t *var);
typedef void (*yalps_milptree_consumed_fn)(void *user, int32_t model, double eval, int32_t n_cuts, const int32_t *cut_sign,
                                           const int32_t *cut_var, const double *cut_val);
int32_t yalps_milptree_search(int32_t count, const int32_t *width, const int32_t *height, const int32_t *root_status,
                              const double *root_result, const double *root_col0, const int32_t *root_pos,
                              const int32_t *root_var, const int64_t *int_offsets, const int32_t *integers,
                              const double *sign, const double *precision, const double *tolerance,
                              const double *timeout_ms, const double *maxIterations, int32_t arena, int32_t arena_max,
                              yalps_milptree_eval_fn eval, yalps_milptree_consumed_fn consumed, void *user,
                              int32_t *status_out, double *result_out, int32_t *height_out, double *col0_out,
                              int32_t *pos_out, int32_t *var_out, int64_t *stats_out, int64_t *reruns_out);

/* Text about the last solve: "launches=.. reruns=.. overflows=.. gpu_us=.. rerun_trees=[..]", then one line per launch with
 * the kernel's spelling, its size class, tree (or LP) count, grid, LDS bytes, history and arena capacity.  Writes at most
 * len - 1 characters and returns the length of the whole text (>= len: cut, call again with a larger buffer). */
int32_t yalps_milptree_info(const yalps_milptree *b, char *buf, int32_t len);

#ifdef __cplusplus
}
#endif
#endif /* YALPS_MILPTREE_H */
