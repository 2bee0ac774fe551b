// lp_dense_kernel.cuh -- a batch of dense LPs of ONE shape read straight from strided device operands, answers written as dense device rows
// Part of libyalps_lpdense.so; included by lp_dense.hip inside its anonymous namespace (gfx950 only).
#pragma once
#include "dense_tableau.cuh"

// ------------------------------------------------------------------------------------------
// lp_dense_kernel is lp_batch_kernel with another first and another last step: fill builds the tableau from the operands where
// they lie -- no cell list, no host pass -- and after writes row i of the outputs (both dense_tableau.cuh); in between the same
// work queue (wg_queue.cuh), wg_simplex unchanged, the same outputs.  What this family adds to the tableau's rules:
//   after  the read-out of x[count][n] and objective[count]; what it reads -- the LP's result, the permutations, column 0 -- it
//          reads where the queue has just written them, behind a barrier of its own.  Skipped, but for that barrier, where the
//          history was full: the rerun writes the row.  Then, where the call asks for them, row i of the marginals (below).
// The three families, each in a code object of its own: lp_dense_kernel (x >= 0), lp_dense_bounds_kernel (lb / ub),
// lp_dense_free_kernel (free variables, with or without lb / ub).
// ------------------------------------------------------------------------------------------
struct DenseCall : DenseDesc {
    double *x;                    // [count][n]
    double *objective;            // [count]
    double *ineqlin;              // [count][m_ub]  the marginals: nullptr where the call does not ask for them
    double *eqlin;                // [count][m_eq]
    double *reduced;              // [count][n]
    double *upper;                // [count][n_upper]  the bound rows' marginals, or nullptr (the bounded and the free kernels)
};

struct DenseLaunch : QueueLaunch {
    const DenseCall *call;
};

// min(row0[c], 0) as np.minimum gives it: a NaN stays a NaN (this is not fmin); c >= 1
__device__ __forceinline__ double dense_cost(const double *mat, int c) {
    const double v = mat[c - 1];
    return v < 0.0 ? v : (v == v ? 0.0 : v);
}
// cost_nb(v): cost at the column variable v ended in, 0 where it is basic
__device__ __forceinline__ double dense_cost_nb(const double *mat, const int32_t *pos, int w, int v) {
    const int p = pos[v];
    return p < w ? dense_cost(mat, p) : 0.0;
}
// y_r of tableau row r: -cost at the column its slack ended in, 0 where the slack is basic
__device__ __forceinline__ double dense_row_dual(const double *mat, const int32_t *pos, int w, int r) {
    const int p = pos[w + r];
    return p < w ? -dense_cost(mat, p) : 0.0;
}

// Row i of the marginals, d(objective) / d(bound) in the caller's direction (s = sign): sensitivity_of's `dual` and
// `reduced_cost` (yalps_amd/sensitivity.py) of the equivalent model, read off the final row 0 -- mat[c - 1] for column c >= 1 --
// and the final positionOfVariable.  Anything but optimal: NaN.
//   ineqlin[r] = s * y(1 + r) + 0.0
//   eqlin[k]   = s * (y(1 + m_ub + 2k) - y(2 + m_ub + 2k)) + 0.0     the upper row minus the negated one: both slacks can be
//                                                                    non-basic at once
//   upper[t]   = s * y(1 + m_ub + 2 m_eq + t) + 0.0                  (bounds) ineqlin's formula on bound row t
//   reduced[j] = s * cost(pos[j + 1]) + 0.0 where variable j is non-basic, else +0.0; of a free variable
//                s * (cost_nb(1 + j) - cost_nb(twin[j])) + 0.0: the full signed reduced cost
// (+ 0.0 turns -0.0 into +0.0.)  Selects, negations, one subtraction, products with +-1: one lane per element, the lanes
// striding as x's do; every lane of the workgroup calls it, under a condition all share (a branch on the output's pointer);
// no LDS, no barrier.
// Inlined into the read-out: it cost the plain instantiations two VGPRs and no scratch; out of line (as sens_epilogue,
// lp_sens_kernel.cuh) there was a call and nothing to buy.
template <int T, class F>
__device__ __forceinline__ void dense_marginals(const DenseCall *d, const int32_t *pos, const double *mat, long long i, int w, bool optimal) {
    const int tid = threadIdx.x, n = F::free ? d->n : w - 1, m_ub = d->m_ub, m_eq = d->m_eq;
    const double sign = d->sign, nan = __longlong_as_double(0x7ff8000000000000ll);
    auto rows = [&](double *out, int count, int first) { // one row per element
        out += i * count;
        for (int r = tid; r < count; r += T) out[r] = optimal ? sign * dense_row_dual(mat, pos, w, first + r) + 0.0 : nan;
    };
    if (double *out = d->ineqlin) rows(out, m_ub, 1);
    if (double *out = d->eqlin) {
        out += i * m_eq;
        for (int k = tid; k < m_eq; k += T) {
            const int r = 1 + m_ub + 2 * k;
            out[k] = optimal ? sign * (dense_row_dual(mat, pos, w, r) - dense_row_dual(mat, pos, w, r + 1)) + 0.0 : nan;
        }
    }
    if (double *out = d->reduced) {
        out += i * n;
        for (int j = tid; j < n; j += T) {
            double v = nan;
            if (optimal) {
                int tj = -1;
                if constexpr (F::free) tj = d->twin[j];
                if (tj >= 0) {
                    v = sign * (dense_cost_nb(mat, pos, w, j + 1) - dense_cost_nb(mat, pos, w, tj)) + 0.0;
                } else {
                    const int p = pos[j + 1];
                    v = p < w ? sign * dense_cost(mat, p) + 0.0 : 0.0;
                }
            }
            out[j] = v;
        }
    }
    if constexpr (F::bounds)
        if (double *out = d->upper) rows(out, d->n_upper, 1 + m_ub + 2 * m_eq);
}

// DenseJob::after behind its barrier: row i of x, objective and the marginals
template <int T, class F>
__device__ __forceinline__ void dense_lp_readout(const DenseCall *d, const int32_t *pos, const int32_t *var, const double *result, const double *mat,
                                                 const double *rhs, long long i, int w, int h, int status) {
    const int n = F::free ? d->n : w - 1;
    DenseLow low{};
    if constexpr (F::bounds) low = dense_low<F>(*d, i);
    const double objective = dense_readout<T, F, false>(d->x + i * n, n, rhs, pos, var, w, h, status == YALPS_OPTIMAL, status == YALPS_UNBOUNDED,
                                                        result, d->sign, d->precision, low, d->c.p + i * d->c.sb, d->c.sr);
    if (threadIdx.x == 0) d->objective[i] = objective;
    dense_marginals<T, F>(d, pos, mat, i, w, status == YALPS_OPTIMAL);
}
template <int T, class F>
__device__ __attribute__((noinline)) void dense_lp_readout_call(const DenseCall *d, const int32_t *pos, const int32_t *var, const double *result,
                                                                const double *mat, const double *rhs, long long i, int w, int h, int status) {
    dense_lp_readout<T, F>(d, pos, var, result, mat, rhs, i, w, h, status);
}

template <class F, bool OUTLINE = false>
struct DenseJob : DenseJobBase<F, OUTLINE> {
    const DenseLaunch &L;
    __device__ __forceinline__ explicit DenseJob(const DenseLaunch &launch) : DenseJobBase<F, OUTLINE>(launch.call), L(launch) {}

    // Every lane; the barrier is met whatever the status.
    template <int T>
    __device__ __forceinline__ void after(const QueueItem &it, int status, const double *mat, const double *rhs, int) const {
        __syncthreads(); // the queue's copies of pos / var / col0 and lane T - 1's result are written
        if (status == WG_HISTORY_FULL) return;
        const DenseCall *call = static_cast<const DenseCall *>(this->d);
        const int i = this->idx;
        if constexpr (OUTLINE) dense_lp_readout_call<T, F>(call, L.pos + it.perm_off, L.var + it.perm_off, L.result + i, mat, rhs, i, it.w, it.h, status);
        else dense_lp_readout<T, F>(call, L.pos + it.perm_off, L.var + it.perm_off, L.result + i, mat, rhs, i, it.w, it.h, status);
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_dense_kernel(DenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJob<DenseTraits<false, false, false>>(L));
}

// the same queue with bounds; instantiated by lp_dense_bounds.hip alone (libyalps_lpdense_bounds.so)
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_dense_bounds_kernel(DenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJob<DenseTraits<true, false, false>>(L));
}

// and with free variables; instantiated by lp_dense_free.hip alone (libyalps_lpdense_free.so).  Its fill and its read-out are
// calls: with both inlined their registers came on top of wg_simplex's in the allocator's eyes and the <1024,check> HBM form
// spilled to scratch, and with the read-out alone out of line it still spilled two registers.
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_dense_free_kernel(DenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJob<DenseTraits<true, true, false>, true>(L));
}
