// milp_tree_rules.cuh -- the search of branch and cut (src/branchAndCut.ts:64-85, :89-176) on a flat arena, host and device.
// Included at file scope by milp_tree.hip (libyalps_milptree.so): milp_tree_kernel's step between two nodes and
// yalps_milptree_search run THIS text.  Plain C++ without containers; it also compiles with g++ alone when __host__ and
// __device__ are defined empty (tools/milp_tree_rules_check.cc).  The rules are milp_search.inc's, restated on arrays:
//   heap      (eval, slot) pairs under heapq's rules (CPython Lib/heapq.py): _siftdown asks `newitem < parent`, _siftup moves
//             the smaller child up all the way to a leaf -- the RIGHT one unless left < right -- and then sifts down again.
//             Only `eval` is compared, with <, so ties and -0.0 against +0.0 keep heapq's order.
//   slots     a frontier node's cut list, at most 2 * n_integers cuts (one per variable and direction: a child drops its
//             parent's cut on the branched variable in its own direction).  A popped node keeps its slot until its children are
//             built, then the slot goes back on the free list.
//   arena     `cap` heap entries and cap + 1 slots (the one more is the popped node's).  A push into a full heap ends the tree
//             with MT_ARENA_FULL and writes nothing.
// The device reads no clock: of `timeout` only "timed out before the first pop" (timeout <= 0) reaches this code.
#pragma once
#include <math.h>
#include <stdint.h>

#define MT_OPTIMAL 0
#define MT_INFEASIBLE 1
#define MT_TIMEDOUT 4       /* YALPS_MILPBATCH_TIMEDOUT */
#define MT_HIST_FULL (-100) /* WG_HISTORY_FULL: a node's pivot history was too short */
#define MT_ARENA_FULL (-101)
#define MT_INCUMBENT 1      /* mt_consume: the node is the new best solution */

struct MtTree {              // what a tree is given
    int32_t w, nints;
    const int32_t *ints;
    double sign, precision, tolerance, max_iter;
    int32_t timedout;        // timeout <= 0
};

struct MtState {             // what a tree is at between two nodes (88 bytes, 11 doubles)
    double best_eval, threshold, iter, cur_eval, result;
    long long used, pivots;
    int32_t heap_n, free_n, found, status, cur_slot, best_height, finished, pad_;
};

struct MtArena {
    MtState *state;
    double *heap_eval, *cut_val;
    int32_t *heap_slot, *free_list, *slot_n, *cut_sv; // cut_sv: (sign, variable) pairs
    int32_t cap, maxcuts;
};

__host__ __device__ inline size_t mt_arena_doubles(int32_t cap, int32_t maxcuts) {
    const size_t slots = (size_t)cap + 1, cuts = slots * (size_t)maxcuts;
    const size_t ints = (size_t)cap + 2 * slots + 2 * cuts;
    return sizeof(MtState) / sizeof(double) + (size_t)cap + cuts + (ints + 1) / 2;
}

__host__ __device__ inline MtArena mt_arena_bind(double *base, int32_t cap, int32_t maxcuts) {
    const size_t slots = (size_t)cap + 1, cuts = slots * (size_t)maxcuts;
    MtArena a;
    a.state = reinterpret_cast<MtState *>(base);
    a.heap_eval = base + sizeof(MtState) / sizeof(double);
    a.cut_val = a.heap_eval + cap;
    a.heap_slot = reinterpret_cast<int32_t *>(a.cut_val + cuts);
    a.free_list = a.heap_slot + cap;
    a.slot_n = a.free_list + slots;
    a.cut_sv = a.slot_n + slots;
    a.cap = cap;
    a.maxcuts = maxcuts;
    return a;
}

// ---- heapq ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void mt_siftdown(const MtArena &a, int32_t startpos, int32_t pos) {
    const double e = a.heap_eval[pos];
    const int32_t s = a.heap_slot[pos];
    while (pos > startpos) {
        const int32_t parent = (pos - 1) >> 1;
        if (e < a.heap_eval[parent]) {
            a.heap_eval[pos] = a.heap_eval[parent];
            a.heap_slot[pos] = a.heap_slot[parent];
            pos = parent;
            continue;
        }
        break;
    }
    a.heap_eval[pos] = e;
    a.heap_slot[pos] = s;
}
__host__ __device__ inline void mt_siftup(const MtArena &a, int32_t pos, int32_t endpos) {
    const int32_t startpos = pos;
    const double e = a.heap_eval[pos];
    const int32_t s = a.heap_slot[pos];
    int32_t child = 2 * pos + 1;
    while (child < endpos) {
        const int32_t right = child + 1;
        if (right < endpos && !(a.heap_eval[child] < a.heap_eval[right])) child = right;
        a.heap_eval[pos] = a.heap_eval[child];
        a.heap_slot[pos] = a.heap_slot[child];
        pos = child;
        child = 2 * pos + 1;
    }
    a.heap_eval[pos] = e;
    a.heap_slot[pos] = s;
    mt_siftdown(a, startpos, pos);
}
// 0: the heap is full, nothing was written
__host__ __device__ inline int mt_heap_push(const MtArena &a, double eval, int32_t slot) {
    MtState &S = *a.state;
    if (S.heap_n >= a.cap) return 0;
    a.heap_eval[S.heap_n] = eval;
    a.heap_slot[S.heap_n] = slot;
    S.heap_n++;
    mt_siftdown(a, 0, S.heap_n - 1);
    return 1;
}
__host__ __device__ inline void mt_heap_pop(const MtArena &a, double *eval, int32_t *slot) {
    MtState &S = *a.state;
    const int32_t last = --S.heap_n;
    const double le = a.heap_eval[last];
    const int32_t ls = a.heap_slot[last];
    if (last == 0) {
        *eval = le, *slot = ls;
        return;
    }
    *eval = a.heap_eval[0], *slot = a.heap_slot[0];
    a.heap_eval[0] = le;
    a.heap_slot[0] = ls;
    mt_siftup(a, 0, last);
}

// ---- slots ------------------------------------------------------------------------------------------------------------
__host__ __device__ inline void mt_reset(const MtArena &a) {
    MtState &S = *a.state;
    S.heap_n = 0;
    S.free_n = a.cap + 1;
    for (int32_t k = 0; k <= a.cap; k++) a.free_list[k] = a.cap - k; // (slot 0 is handed out first)
}
__host__ __device__ inline int32_t mt_slot_alloc(const MtArena &a) {
    MtState &S = *a.state;
    if (S.free_n <= 0) return -1;
    const int32_t s = a.free_list[--S.free_n];
    a.slot_n[s] = 0;
    return s;
}
__host__ __device__ inline void mt_slot_free(const MtArena &a, int32_t s) { a.free_list[a.state->free_n++] = s; }
// 0: the slot is full, nothing was written
__host__ __device__ inline int mt_slot_add(const MtArena &a, int32_t s, int32_t sign, int32_t variable, double value) {
    const int32_t n = a.slot_n[s];
    if (n >= a.maxcuts) return 0;
    const size_t at = (size_t)s * a.maxcuts + n;
    a.cut_sv[2 * at] = sign;
    a.cut_sv[2 * at + 1] = variable;
    a.cut_val[at] = value;
    a.slot_n[s] = n + 1;
    return 1;
}

// ---- src/branchAndCut.ts:64-85 -------------------------------------------------------------------------------------------
__host__ __device__ inline double mt_js_round(double x) { // Math.round
    if (!(fabs(x) < INFINITY)) return x;
    const double f = floor(x);
    const double r = (x - f >= 0.5) ? f + 1.0 : f;
    return r == 0.0 ? copysign(0.0, x) : r; // (-0 on [-0.5, -0]; the caller takes fabs(val - round), which cannot tell)
}
__host__ __device__ inline double mt_most_fractional(const MtTree &T, const double *col0, const int32_t *pos, int32_t *variable,
                                                     double *value) {
    double highest = 0.0, val_best = 0.0;
    int32_t var_best = 0;
    for (int32_t i = 0; i < T.nints; i++) {
        const int32_t row = pos[T.ints[i]] - T.w;
        if (row < 0) continue;
        const double val = col0[row];
        const double frac = fabs(val - mt_js_round(val));
        if (frac > highest) { // (strict: the first of equals wins, a NaN never does)
            highest = frac;
            var_best = T.ints[i];
            val_best = val;
        }
    }
    *variable = var_best;
    *value = val_best;
    return highest;
}

__host__ __device__ inline void mt_finish(const MtArena &a, int32_t status, double result) {
    MtState &S = *a.state;
    S.finished = 1;
    S.status = status;
    S.result = result;
}

// a new frontier node: `eval`, the cuts of slot `from` that `keep` lets through (0: none, +1 / -1: all but those on
// `variable` of that direction's opposite side, :146-151), then the new cut LAST.  0: the arena is full, nothing is pushed.
__host__ __device__ inline int mt_push_node(const MtArena &a, double eval, int32_t from, int upper, int32_t variable, int32_t sign,
                                            double value) {
    if (a.state->heap_n >= a.cap) return 0;
    const int32_t s = mt_slot_alloc(a);
    if (s < 0) return 0;
    if (from >= 0) {
        const int32_t n = a.slot_n[from];
        for (int32_t q = 0; q < n; q++) {
            const size_t at = (size_t)from * a.maxcuts + q;
            const int32_t dir = a.cut_sv[2 * at], v = a.cut_sv[2 * at + 1];
            if (v == variable && (dir < 0) == (upper != 0)) continue; // dir < 0 ? cutsLower : cutsUpper
            if (!mt_slot_add(a, s, dir, v, a.cut_val[at])) return 0;
        }
    }
    if (!mt_slot_add(a, s, sign, variable, value)) return 0;
    return mt_heap_push(a, eval, s);
}

// :89-120 after simplex() on the root.  Leaves the tree finished or with its first two children pushed.
__host__ __device__ inline void mt_begin(const MtTree &T, const MtArena &a, int32_t root_status, double root_result,
                                         const double *root_col0, const int32_t *root_pos) {
    MtState &S = *a.state;
    S.best_eval = INFINITY;
    S.threshold = 0.0;
    S.iter = 0.0;
    S.cur_eval = 0.0;
    S.result = NAN;
    S.used = S.pivots = 0;
    S.found = S.finished = S.best_height = S.pad_ = 0;
    S.status = 3;
    S.cur_slot = -1;
    mt_reset(a);
    if (root_status != MT_OPTIMAL || T.nints == 0) return mt_finish(a, root_status, root_result);
    int32_t variable = 0;
    double value = 0.0;
    const double frac = mt_most_fractional(T, root_col0, root_pos, &variable, &value);
    if (frac <= T.precision) return mt_finish(a, MT_OPTIMAL, root_result); // :98
    if (!mt_push_node(a, root_result, -1, 1, variable, -1, ceil(value)) ||
        !mt_push_node(a, root_result, -1, 0, variable, 1, floor(value)))
        return mt_finish(a, MT_ARENA_FULL, NAN);
    S.threshold = root_result * (1.0 - T.sign * T.tolerance); // :114
}

// :122-124, and :166-175 where the loop ends.  1: the node of state->cur_slot is to be evaluated; 0: the tree is finished.
__host__ __device__ inline int mt_next(const MtTree &T, const MtArena &a) {
    MtState &S = *a.state;
    if (S.finished) return 0;
    if (S.iter < T.max_iter && S.heap_n > 0 && S.best_eval >= S.threshold && !T.timedout) {
        mt_heap_pop(a, &S.cur_eval, &S.cur_slot);
        if (!(S.cur_eval > S.best_eval)) return 1;
    }
    const bool unfinished = (T.timedout || S.iter >= T.max_iter) && S.heap_n > 0 && S.best_eval >= S.threshold;
    mt_finish(a, unfinished ? MT_TIMEDOUT : (S.found ? MT_OPTIMAL : MT_INFEASIBLE), S.found ? S.best_eval : NAN);
    return 0;
}

// :127-163 with the popped node solved: status, result and -- of an optimal node -- its column 0 and positionOfVariable.
// MT_INCUMBENT: the caller keeps the node's tableau as the best one.  MT_ARENA_FULL: the tree is finished with that code.
__host__ __device__ inline int mt_consume(const MtTree &T, const MtArena &a, int32_t status, double result, const double *col0,
                                          const int32_t *pos, int32_t height) {
    MtState &S = *a.state;
    int ret = 0;
    S.used++;
    if (status == MT_OPTIMAL && result < S.best_eval) {
        int32_t variable = 0;
        double value = 0.0;
        const double frac = mt_most_fractional(T, col0, pos, &variable, &value);
        if (frac <= T.precision) { // :132-139
            S.found = 1;
            S.best_eval = result;
            S.best_height = height;
            ret = MT_INCUMBENT;
        } else if (!mt_push_node(a, result, S.cur_slot, 1, variable, -1, ceil(value)) || // cutsUpper first (:155-156)
                   !mt_push_node(a, result, S.cur_slot, 0, variable, 1, floor(value))) {
            mt_finish(a, MT_ARENA_FULL, NAN);
            return MT_ARENA_FULL;
        }
    }
    mt_slot_free(a, S.cur_slot);
    S.cur_slot = -1;
    S.iter += 1.0;
    return ret;
}
