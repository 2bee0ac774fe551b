// milp_dense_kernel.cuh -- the two kernels of libyalps_milpdense.so around milp_tree_kernel: the root LPs of a batch of dense
// MILPs of ONE shape read straight from strided device operands, and solution() of every tree written as dense device rows.
// Included by milp_dense.hip inside its anonymous namespace (gfx950 only), after milp_tree_rules.cuh (file scope) and wg_simplex.cuh.
#pragma once
#include "wg_queue.cuh"

// ------------------------------------------------------------------------------------------
// All MILPs of a call share one shape and one set of integer and binary variables: n variables x >= 0, m_ub rows
// A_ub x <= b_ub, m_eq rows A_eq x = b_eq, n_bin binary variables; w = n + 1, h0 = 1 + m_ub + 2 * m_eq, h = h0 + n_bin.
// milp_dense_root_kernel is lp_dense_kernel's job with a longer first step and no last one:
//   fill   tableauModel's initial tableau (src/tableau.ts:47-137).  Rows 0 .. h0 - 1 are DenseJob::fill's (lp_dense_kernel.cuh):
//          row 0 +0.0, sign * c[j] (a product); row 1 + i b_ub[i], A_ub[i, j]; rows 1 + m_ub + 2k and the one after it
//          b_eq[k], A_eq[k, j] and their IEEE negations.  Row h0 + q, for the q-th binary variable in ascending index
//          (src/tableau.ts:122-128): column 0 1.0, the column of variable bin[q] 1.0, the rest +0.0.  Identity permutations,
//          the padding columns of the pitch +0.0.  Values are taken as they lie in memory.
//          Lanes run along the columns of a row, so an operand whose column stride is 1 is read coalesced.
//   after  nothing: the pass runs with kept tableaux (milp_tree_kernel cuts its nodes from them), and x is written after the
//          trees, by milp_dense_solution_kernel.
// The call's description lies in device memory (one MilpDenseCall per call, the binary list behind it), not in the kernel's
// arguments, as DenseCall does: five operands with three 64-bit strides each would sit in scalar registers through the solve.
// ------------------------------------------------------------------------------------------
struct MilpDenseOperand {
    const double *p;              // element (i, r, c) at p[i * sb + r * sr + c * sc]; a vector has sc = 0 and is indexed by r
    long long sb, sr, sc;
};

struct MilpDenseCall {
    int32_t n, m_ub, m_eq, n_bin;
    int32_t aux_hbm, pad_;        // aux_hbm: HBM form, colbuf / prow behind the tableau in the workspace
    double sign;                  // +1 maximise, -1 minimise
    double precision, max_pivots;
    MilpDenseOperand c, A_ub, b_ub, A_eq, b_eq; // c and the b's: (batch, row) = (i, j), sc unused
    const int32_t *bin;           // [n_bin] 0-based variable indices, ascending
};

struct MilpDenseLaunch : QueueLaunch {
    const MilpDenseCall *call;
};

struct MilpDenseJob : QueueJobBase {
    const MilpDenseCall *d;
    int idx;
    __device__ __forceinline__ explicit MilpDenseJob(const MilpDenseLaunch &launch) : d(launch.call), idx(0) {}
    __device__ __forceinline__ QueueItem item(int i) {
        idx = i;
        const int w = d->n + 1, h = 1 + d->m_ub + 2 * d->m_eq + d->n_bin, heven = (h + 1) & ~1;
        return QueueItem{w, h, (long long)((size_t)i * heven), (long long)((size_t)i * ((size_t)w + h)), d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int i, const QueueItem &it) const { return (long long)((size_t)i * it.w * it.h); }

    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        const int tid = threadIdx.x, w = it.w, h = it.h, n = w - 1, m_ub = d->m_ub, h0 = h - d->n_bin;
        const long long i = idx;
        const double sign = d->sign;
        // a group of Uc lanes per row, the lanes along its columns (lane `lp` of a row, where it exists, writes column 0)
        const int Uc = wg_unit_lanes(lp + 1, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
        for (int r = cg0; r < h; r += CG) {
            double *dst = mat + (size_t)r * lp;
            if (r >= h0) { // a binary variable's row: x <= 1   (r is the same for the lanes of a group)
                const int jb = d->bin[r - h0];
                for (int c = cu0; c <= lp; c += Uc) {
                    if (c == lp)
                        rhs[r] = 1.0;
                    else
                        dst[c] = c == jb ? 1.0 : 0.0;
                }
                continue;
            }
            const double *a, *b; // the row's coefficients, and its right-hand side
            long long sc;
            bool neg = false;
            if (r == 0) {
                a = d->c.p + i * d->c.sb;
                sc = d->c.sr;
                b = nullptr;
            } else if (r <= m_ub) {
                a = d->A_ub.p + i * d->A_ub.sb + (long long)(r - 1) * d->A_ub.sr;
                sc = d->A_ub.sc;
                b = d->b_ub.p + i * d->b_ub.sb + (long long)(r - 1) * d->b_ub.sr;
            } else {
                const int k = (r - 1 - m_ub) >> 1;
                neg = ((r - 1 - m_ub) & 1) != 0;
                a = d->A_eq.p + i * d->A_eq.sb + (long long)k * d->A_eq.sr;
                sc = d->A_eq.sc;
                b = d->b_eq.p + i * d->b_eq.sb + (long long)k * d->b_eq.sr;
            }
            for (int c = cu0; c <= lp; c += Uc) {
                if (c == lp) {
                    rhs[r] = r == 0 ? 0.0 : (neg ? -*b : *b);
                } else if (c >= n) {
                    dst[c] = 0.0;
                } else {
                    const double v = a[(long long)c * sc];
                    dst[c] = r == 0 ? sign * v : (neg ? -v : v);
                }
            }
        }
        for (int p = tid; p < w + h; p += T) {
            pos[p] = p;
            var[p] = p;
        }
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_dense_root_kernel(MilpDenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, MilpDenseJob(L));
}

// ------------------------------------------------------------------------------------------
// milp_dense_solution_kernel: solution() (src/YALPS.ts:8-50) of every tree, one workgroup per tree, the lanes striding along
// the variables.  Tree i's status, result and best height are read where milp_tree_kernel left them (best_h == nullptr: the
// call has no integer variable, there was no tree pass, status / result are the root pass's).  Column 0 and the permutations
// of the best tableau: the tree's output slice where best_h > 0, else the root's -- a root that is not optimal, a root that is
// already integral, and a search that found nothing (src/branchAndCut.ts:119).
//   "optimal", or "timedout" with a result that is not NaN: x[j] = col0[pos[j + 1] - w] where variable j is basic, above
//       precision rounded to it, anything else +0.0; objective = -sign * result
//   "unbounded": +0.0, +inf at the unbounded variable; objective = sign * inf
//   anything else: NaN.  A status that is none of the public ones (the tree's frontier outgrew the largest arena and the host
//       gave it up) also gets status_out = overflow and zero counts: the caller solves that row another way.
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
};

template <int T>
__global__ __launch_bounds__(T) void milp_dense_solution_kernel(MilpSolutionArgs a) {
    const int tid = threadIdx.x, n = a.n, w = n + 1;
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
    const double sign = a.sign, p = a.precision;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    double *x = a.x ? a.x + i * (size_t)n : nullptr;
    double objective = nan;
    if (st == YALPS_OPTIMAL || (st == MT_TIMEDOUT && has)) {
        if (x)
            for (int j = tid; j < n; j += T) {
                const int row = pos[j + 1] - w;
                const double v = (unsigned)row < (unsigned)h ? col0[row] : 0.0;
                x[j] = v > p ? round_to_precision(v, p) : 0.0;
            }
        objective = -sign * res;
    } else if (st == YALPS_UNBOUNDED) {
        const int at = (int)res;
        const int v = (unsigned)at < (unsigned)(w + h) ? var[at] - 1 : -1;
        if (x)
            for (int j = tid; j < n; j += T) x[j] = j == v ? INFINITY : 0.0;
        objective = sign * INFINITY;
    } else {
        if (x)
            for (int j = tid; j < n; j += T) x[j] = nan;
    }
    if (tid == 0) {
        if (a.objective) a.objective[i] = objective;
        if (st < 0 || st > MT_TIMEDOUT) {
            if (a.status_out) a.status_out[i] = a.overflow;
            if (a.nodes_out) a.nodes_out[i] = 0;
            if (a.node_pivots_out) a.node_pivots_out[i] = 0;
        }
    }
}
