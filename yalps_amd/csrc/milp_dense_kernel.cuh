// milp_dense_kernel.cuh -- the two kernels of libyalps_milpdense.so around milp_tree_kernel: the root LPs of a batch of dense
// MILPs of ONE shape read straight from strided device operands, and solution() of every tree written as dense device rows.
// Included by milp_dense.hip inside its anonymous namespace (gfx950 only), after milp_tree_rules.cuh (file scope) and wg_simplex.cuh.
#pragma once
#include "dense_tableau.cuh"

// ------------------------------------------------------------------------------------------
// All MILPs of a call share one shape and one set of integer and binary variables.  milp_dense_root_kernel is lp_dense_kernel's
// job with the binary rows (dense_tableau.cuh) and no last step: the pass runs with kept tableaux (milp_tree_kernel cuts its
// nodes from them), and x is written after the trees, by milp_dense_solution_kernel.  The description is a DenseDesc with the
// lists it points to behind it; `bin`, `upper_idx`, the kind bytes and the twins are host decisions.
// ------------------------------------------------------------------------------------------
struct MilpDenseLaunch : QueueLaunch {
    const DenseDesc *call;
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_dense_root_kernel(MilpDenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJobBase<DenseTraits<false, false, true>>(L.call));
}

// ------------------------------------------------------------------------------------------
// milp_dense_solution_kernel: the read-out (dense_tableau.cuh) of every tree, one workgroup per tree.  Tree i's status, result
// and best height are read where milp_tree_kernel left them (best_h == nullptr: the call has no integer variable, there was no
// tree pass, status / result are the root pass's).  Column 0 and the permutations of the best tableau: the tree's output slice
// where best_h > 0, else the root's -- a root that is not optimal, a root that is already integral, and a search that found
// nothing (src/branchAndCut.ts:119).  "timedout" with a result that is not NaN reads as "optimal".  A status that is none of the
// public ones (the tree's frontier outgrew the largest arena and the host gave it up) is NaN and also gets status_out = overflow
// and zero counts: the caller solves that row another way.
// status, best_h and the result's NaN-ness go through readfirstlane: every branch on them is the whole workgroup's.
// Launched on the stream behind the last tree pass and the device-to-device copies of status and counts; it reads every tree
// of the call, whichever pass finished it.
// ------------------------------------------------------------------------------------------
struct MilpSolutionArgs {
    int32_t n, h0, hmax, overflow; // h0: root height; hmax = h0 + 2 * n_int: the tree slices' stride; overflow: its public code
    double sign, precision;
    const int32_t *status;        // [count]
    const double *result;         // [count]
    const int32_t *best_h;        // [count] or nullptr
    const double *root_col0, *tree_col0;
    const int32_t *root_pos, *root_var, *tree_pos, *tree_var;
    double *x, *objective;        // [count][n], [count]; nullptr: not wanted
    int32_t *status_out;          // the three below: already copied, patched for a tree the host gave up; nullptr: not wanted
    long long *nodes_out, *node_pivots_out;
    // with bounds and with free variables
    DenseOperand c, lb;           // lb.p = nullptr: absent
    const uint8_t *kind;          // [n]
    // with free variables
    int32_t n_free, pad_;
    const int32_t *twin;          // [n]
};

template <int T, class F>
__device__ __forceinline__ void milp_dense_solution(const MilpSolutionArgs &a) {
    const int n = a.n, w = n + 1 + (F::free ? a.n_free : 0);
    const size_t i = blockIdx.x;
    const int st = __builtin_amdgcn_readfirstlane(a.status[i]);
    const int bh = a.best_h ? __builtin_amdgcn_readfirstlane(a.best_h[i]) : 0;
    const double res = a.result[i];
    const int has = __builtin_amdgcn_readfirstlane(res == res ? 1 : 0);
    const bool tree = bh > 0;
    const int h = tree ? bh : a.h0;
    const size_t hs = tree ? (size_t)a.hmax : (size_t)a.h0; // the slice's stride follows its buffer
    const double *col0 = (tree ? a.tree_col0 : a.root_col0) + i * ((hs + 1) & ~(size_t)1);
    const int32_t *pos = (tree ? a.tree_pos : a.root_pos) + i * ((size_t)w + hs);
    const int32_t *var = (tree ? a.tree_var : a.root_var) + i * ((size_t)w + hs);
    DenseLow low{};
    if constexpr (F::bounds) low = dense_low<F>(a, (long long)i);
    const double objective = dense_readout<T, F, true>(a.x ? a.x + i * (size_t)n : nullptr, n, col0, pos, var, w, h,
                                                       st == YALPS_OPTIMAL || (st == MT_TIMEDOUT && has), st == YALPS_UNBOUNDED, a.result + i,
                                                       a.sign, a.precision, low, a.c.p + (long long)i * a.c.sb, a.c.sr);
    if (threadIdx.x == 0) {
        if (a.objective) a.objective[i] = objective;
        if (st < 0 || st > MT_TIMEDOUT) {
            if (a.status_out) a.status_out[i] = a.overflow;
            if (a.nodes_out) a.nodes_out[i] = 0;
            if (a.node_pivots_out) a.node_pivots_out[i] = 0;
        }
    }
}

template <int T>
__global__ __launch_bounds__(T) void milp_dense_solution_kernel(MilpSolutionArgs a) {
    milp_dense_solution<T, DenseTraits<false, false, true>>(a);
}
