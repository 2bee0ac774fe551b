// lp_dense_kernel.cuh -- a batch of dense LPs of ONE shape read straight from strided device operands, answers written as dense device rows
// Part of libyalps_lpdense.so; included by lp_dense.hip inside its anonymous namespace (gfx950 only).
#pragma once
#include "wg_queue.cuh"

// ------------------------------------------------------------------------------------------
// All LPs of a call share one shape: n variables x >= 0, m_ub rows A_ub x <= b_ub, m_eq rows A_eq x = b_eq; w = n + 1,
// h = 1 + m_ub + 2 * m_eq.  lp_dense_kernel is lp_batch_kernel with another first and another last step:
//   fill   builds tableauModel's initial tableau (src/tableau.ts:47-137) from the operands where they lie -- no cell list, no
//          host pass.  Row 0: +0.0, sign * c[j] (a product: -1 * 0.0 is -0.0).  Row 1 + i: b_ub[i], A_ub[i, j].  Rows
//          1 + m_ub + 2k and the one after it: b_eq[k], A_eq[k, j] and their IEEE negations (a zero becomes -0.0, as
//          `m[...] = -coef` makes it).  Identity permutations; the padding columns of the pitch +0.0, as LpJob's zero pass
//          leaves them.  Values are taken as they lie in memory: a NaN or an infinity goes into the tableau.
//          Lanes run along the columns of a row, so an operand whose column stride is 1 is read coalesced.
//   after  does solution()'s work (src/YALPS.ts:8-50) for row i of the outputs x[count][n], objective[count]; what it reads --
//          the LP's result, the permutations, column 0 -- it reads where the queue has just written them, behind a barrier
//          of its own.  Skipped, but for that barrier, where the history was full: the rerun writes the row.
//          Where the call asks for them (a uniform branch on three pointers) it also writes row i of the marginals
//          ineqlin[count][m_ub], eqlin[count][m_eq], reduced[count][n]: sensitivity_of's `dual` and `reduced_cost`
//          (yalps_amd/sensitivity.py) of the equivalent model, read off the final row 0 -- mat[c - 1] for column c >= 1 --
//          and the final positionOfVariable; see marginals() below.
// In between: the same work queue (wg_queue.cuh), wg_simplex unchanged, the same outputs.
// The call's description lies in device memory (one DenseCall per call), not in the kernel's arguments: five operands with
// three 64-bit strides each would sit in scalar registers through the solve.
// ------------------------------------------------------------------------------------------
struct DenseOperand {
    const double *p;              // element (i, r, c) at p[i * sb + r * sr + c * sc]; a vector has sc = 0 and is indexed by r
    long long sb, sr, sc;
};

struct DenseCall {
    int32_t n, m_ub, m_eq, aux_hbm; // aux_hbm: HBM form, colbuf / prow behind the tableau in the workspace
    double sign;                  // +1 maximise, -1 minimise
    double precision, max_pivots;
    DenseOperand c, A_ub, b_ub, A_eq, b_eq; // c and the b's: (batch, row) = (i, j), sc unused
    double *x;                    // [count][n]
    double *objective;            // [count]
    double *ineqlin;              // [count][m_ub]  the marginals: nullptr where the call does not ask for them
    double *eqlin;                // [count][m_eq]
    double *reduced;              // [count][n]
};

struct DenseLaunch : QueueLaunch {
    const DenseCall *call;
};

// min(row0[c], 0) as np.minimum gives it: a NaN stays a NaN (this is not fmin); c >= 1
__device__ __forceinline__ double dense_cost(const double *mat, int c) {
    const double v = mat[c - 1];
    return v < 0.0 ? v : (v == v ? 0.0 : v);
}
// y_r of tableau row r: -cost at the column its slack ended in, 0 where the slack is basic
__device__ __forceinline__ double dense_row_dual(const double *mat, const int32_t *pos, int w, int r) {
    const int p = pos[w + r];
    return p < w ? -dense_cost(mat, p) : 0.0;
}

// Row i of the marginals, d(objective) / d(bound) in the caller's direction (s = sign); anything but optimal: NaN.
//   ineqlin[r] = s * y(1 + r) + 0.0
//   eqlin[k]   = s * (y(1 + m_ub + 2k) - y(2 + m_ub + 2k)) + 0.0     the upper row minus the negated one: both slacks can be
//                                                                    non-basic at once
//   reduced[j] = s * cost(pos[j + 1]) + 0.0 where variable j is non-basic, else +0.0
// (+ 0.0 turns -0.0 into +0.0.)  Selects, negations, one subtraction, products with +-1: one lane per element, the lanes
// striding as x's do; every lane of the workgroup calls it, under a condition all share; no LDS, no barrier.
// Inlined: it costs the six instantiations two VGPRs (101-116 of 128) and no scratch; out of line (as sens_epilogue,
// lp_sens_kernel.cuh) it built to 99-115 and a call, so there was nothing to buy.
template <int T>
__device__ __forceinline__ void dense_marginals(const DenseCall *d, const int32_t *pos, const double *mat, long long i,
                                                       int w, bool optimal) {
    const int tid = threadIdx.x, n = w - 1, m_ub = d->m_ub, m_eq = d->m_eq;
    const double sign = d->sign, nan = __longlong_as_double(0x7ff8000000000000ll);
    if (double *out = d->ineqlin) {
        out += i * m_ub;
        for (int r = tid; r < m_ub; r += T) out[r] = optimal ? sign * dense_row_dual(mat, pos, w, 1 + r) + 0.0 : nan;
    }
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
                const int p = pos[j + 1];
                v = p < w ? sign * dense_cost(mat, p) + 0.0 : 0.0;
            }
            out[j] = v;
        }
    }
}

struct DenseJob : QueueJobBase {
    const DenseLaunch &L;
    const DenseCall *d;
    int idx;
    __device__ __forceinline__ explicit DenseJob(const DenseLaunch &launch) : L(launch), d(launch.call), idx(0) {}
    __device__ __forceinline__ QueueItem item(int i) {
        idx = i;
        const int w = d->n + 1, h = 1 + d->m_ub + 2 * d->m_eq, heven = (h + 1) & ~1;
        return QueueItem{w, h, (long long)((size_t)i * heven), (long long)((size_t)i * ((size_t)w + h)), d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int i, const QueueItem &it) const { return (long long)((size_t)i * it.w * it.h); }

    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        const int tid = threadIdx.x, w = it.w, h = it.h, n = w - 1, m_ub = d->m_ub;
        const long long i = idx;
        const double sign = d->sign;
        // a group of Uc lanes per row, the lanes along its columns (lane `lp` of a row, where it exists, writes column 0)
        const int Uc = wg_unit_lanes(lp + 1, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
        for (int r = cg0; r < h; r += CG) {
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
            double *dst = mat + (size_t)r * lp;
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

    // solution() on the device: row idx of x and objective.  Every lane; the barrier is met whatever the status.
    template <int T>
    __device__ __forceinline__ void after(const QueueItem &it, int status, const double *mat, const double *rhs, int) const {
        __syncthreads(); // the queue's copies of pos / var / col0 and lane T - 1's result are written
        if (status == WG_HISTORY_FULL) return;
        const int tid = threadIdx.x, w = it.w, n = w - 1;
        const long long i = idx;
        double *x = d->x + i * n;
        const double sign = d->sign, p = d->precision;
        const double nan = __longlong_as_double(0x7ff8000000000000ll);
        double objective = nan;
        if (status == YALPS_OPTIMAL) {
            const int32_t *pos = L.pos + it.perm_off;
            for (int j = tid; j < n; j += T) {
                const int row = pos[j + 1] - w;
                const double v = row >= 0 ? rhs[row] : 0.0;
                x[j] = v > p ? round_to_precision(v, p) : 0.0;
            }
            objective = -sign * L.result[i];
        } else if (status == YALPS_UNBOUNDED) {
            const int32_t *var = L.var + it.perm_off;
            const int at = (int)L.result[i];
            const int v = (unsigned)at < (unsigned)(w + it.h) ? var[at] - 1 : -1;
            for (int j = tid; j < n; j += T) x[j] = j == v ? INFINITY : 0.0;
            objective = sign * INFINITY;
        } else {
            for (int j = tid; j < n; j += T) x[j] = nan;
        }
        if (tid == 0) d->objective[i] = objective;
        if (d->ineqlin || d->eqlin || d->reduced) dense_marginals<T>(d, L.pos + it.perm_off, mat, i, w, status == YALPS_OPTIMAL);
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_dense_kernel(DenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJob(L));
}
