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
//
// Bounds (DenseJob<true>, lp_dense_bounds_kernel; the boundless job and its six kernels are compiled without a line of this):
// x >= lb replaces x >= 0 by the substitution x = lb + x', and x[j] <= ub[j] for the n_upper listed variables adds n_upper rows
// below the equality rows, so h = 1 + m_ub + 2 * m_eq + n_upper.
//   shift_sum(a, l), THE order: every product a[j] * l[j] rounded on its own; lane k of ONE wave adds the products of the
//          columns j = k (mod 64) in ascending j to +0.0; then p += shfl_down(p, s) for s = 32, 16, 8, 4, 2, 1; lane 0 holds it.
//          It depends on nothing but a and l: not on T, the LDS / HBM / aux form, wg_unit_lanes, strides or the batch.
//   fill   with lb: a pass of its own in front of the row loop, one wave per operand row, parks the row's shift_sum in the
//          row's rhs slot (both slots of an equality); one barrier; the row loop's column-0 lane then writes b - rhs[r], one
//          subtraction (its negation in the second row of an equality).  Without lb nothing is subtracted.  Coefficients and
//          row 0 are untouched.  Bound row t: ub[j] - lb[j] (or ub[j]) in column 0, 1.0 in column j = upper_idx[t], else +0.0:
//          generated, not read.
//   after  x = x' + lb, one addition per element whatever the status; objective = objective' + shift_sum(c, lb), recomputed
//          here by wave 0 (lane 0 of the workgroup writes it), one addition after the rounding; upper[t] = ineqlin's
//          formula on bound row t.
//
// Free variables (DenseFreeJob, lp_dense_free_kernel; a sibling job, so that DenseJob<false> and DenseJob<true> are compiled from
// the lines they were compiled from): a free variable j is split as x[j] = p[j] - q[j], p, q >= 0.  p keeps column 1 + j, the
// twins q are n_free generated columns behind the n originals in ascending j, so w = 1 + n + n_free; h as with bounds.
//   fill   a twin cell is the IEEE negation of the cell of column 1 + j in the same row -- of the value written there, not a
//          second product: one strided read of the operand at free_idx[c - n] by the lane that owns column c.  In a bound row
//          of a free variable the twin cell is -1.0, in every other bound row +0.0.  lb is not read at a free variable: the
//          effective lower bound there is +0.0, whose product with the coefficient is still formed and added in shift_sum,
//          which runs over the n original columns alone.  The branches are on r (a row group) and on c (a lane), never per LP.
//   after  x[j] = v(p) - v(q), each v today's rule on its own column (basic and above precision: rounded; else +0.0), one
//          subtraction, then + l_eff[j] where lb is given; "unbounded": +inf at the unbounded column, so -inf where that is a
//          twin.  The lane that owns j reads twin[j] (-1, or the twin's column) and, for a free variable, one more pos entry:
//          no barrier and no LDS beyond the bounded job's.
//          reduced[j] of a free variable = s * (cost_nb(1 + j) - cost_nb(twin[j])) + 0.0, cost_nb(v) = cost(pos[v]) where
//          pos[v] < w, else 0: the full signed reduced cost.  The rows' marginals use the new w and are otherwise unchanged.
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
    // bounds: read by DenseJob<true> only (behind everything the boundless kernels read, whose offsets stay)
    DenseOperand lb, ub;          // (batch, row) = (i, j), sc unused; p = nullptr: absent
    int32_t n_upper;              // bound rows; ub is read at upper_idx[0 .. n_upper) only
    const int32_t *upper_idx;     // device, ascending
    double *upper;                // [count][n_upper]  the bound rows' marginals, or nullptr
    // free variables: read by DenseFreeJob only (behind everything the other twelve kernels read, whose offsets stay)
    int32_t n_free;               // twin columns behind the n originals
    const int32_t *free_idx;      // device, ascending: twin t (column 1 + n + t) is the twin of variable free_idx[t]
    const int32_t *twin;          // device, [n]: the twin's column 1 + n + t of a free variable, -1 of any other
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

// shift_sum(a, l) over n columns, the canonical order (above): every lane of a wave calls it, lane 0's value is the sum
__device__ __forceinline__ double dense_shift_sum(const double *a, long long sa, const double *l, long long sl, int n) {
    double p = 0.0;
    for (int j = threadIdx.x & 63; j < n; j += 64) p = p + a[(long long)j * sa] * l[(long long)j * sl];
    for (int s = 32; s > 0; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

// Row i of the bound rows' marginals: upper[t] = s * y(1 + m_ub + 2 m_eq + t) + 0.0, ineqlin's formula; not optimal: NaN
template <int T>
__device__ __forceinline__ void dense_upper_marginals(const DenseCall *d, const int32_t *pos, const double *mat, long long i,
                                                      int w, bool optimal) {
    const int k = d->n_upper, first = 1 + d->m_ub + 2 * d->m_eq;
    const double sign = d->sign, nan = __longlong_as_double(0x7ff8000000000000ll);
    double *out = d->upper + i * k;
    for (int t = threadIdx.x; t < k; t += T) out[t] = optimal ? sign * dense_row_dual(mat, pos, w, first + t) + 0.0 : nan;
}

template <bool BOUNDS>
struct DenseJob : QueueJobBase {
    const DenseLaunch &L;
    const DenseCall *d;
    int idx;
    __device__ __forceinline__ explicit DenseJob(const DenseLaunch &launch) : L(launch), d(launch.call), idx(0) {}
    __device__ __forceinline__ QueueItem item(int i) {
        idx = i;
        const int w = d->n + 1, h = 1 + d->m_ub + 2 * d->m_eq + (BOUNDS ? d->n_upper : 0), heven = (h + 1) & ~1;
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
        const double *lb = nullptr, *ub = nullptr;
        long long lbs = 0, ubs = 0;
        int h0 = h; // the first bound row
        if constexpr (BOUNDS) {
            h0 = h - d->n_upper;
            lbs = d->lb.sr, ubs = d->ub.sr;
            if (d->lb.p) lb = d->lb.p + i * d->lb.sb;
            if (d->ub.p) ub = d->ub.p + i * d->ub.sb;
            if (lb) { // the shifts: one wave per operand row, parked in the row's rhs slot
                const int m_eq = d->m_eq;
                for (int q = tid >> 6; q < m_ub + m_eq; q += T >> 6) {
                    const bool eq = q >= m_ub;
                    const DenseOperand &A = eq ? d->A_eq : d->A_ub;
                    const int k = eq ? q - m_ub : q;
                    const double v = dense_shift_sum(A.p + i * A.sb + (long long)k * A.sr, A.sc, lb, lbs, n);
                    if ((tid & 63) == 0) {
                        if (eq) rhs[1 + m_ub + 2 * k] = rhs[2 + m_ub + 2 * k] = v;
                        else rhs[1 + q] = v;
                    }
                }
                __syncthreads();
            }
        }
        for (int r = cg0; r < h; r += CG) {
            const double *a, *b; // the row's coefficients, and its right-hand side
            long long sc;
            bool neg = false;
            if constexpr (BOUNDS) {
                if (r >= h0) { // a bound row: nothing but column 0 is read
                    const int j = d->upper_idx[r - h0];
                    double *dst = mat + (size_t)r * lp;
                    for (int c = cu0; c <= lp; c += Uc) {
                        if (c == lp) {
                            const double u = ub[(long long)j * ubs];
                            rhs[r] = lb ? u - lb[(long long)j * lbs] : u;
                        } else {
                            dst[c] = c == j ? 1.0 : 0.0;
                        }
                    }
                    continue;
                }
            }
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
                    if constexpr (BOUNDS) {
                        if (lb && r != 0) {
                            const double v = *b - rhs[r];
                            rhs[r] = neg ? -v : v;
                            continue;
                        }
                    }
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
        const double *lb = nullptr; // x = x' + lb, whatever the status
        long long lbs = 0;
        if constexpr (BOUNDS) {
            lbs = d->lb.sr;
            if (d->lb.p) lb = d->lb.p + i * d->lb.sb;
        }
        if (status == YALPS_OPTIMAL) {
            const int32_t *pos = L.pos + it.perm_off;
            for (int j = tid; j < n; j += T) {
                const int row = pos[j + 1] - w;
                const double v = row >= 0 ? rhs[row] : 0.0;
                const double xv = v > p ? round_to_precision(v, p) : 0.0;
                if constexpr (BOUNDS) {
                    x[j] = lb ? xv + lb[(long long)j * lbs] : xv;
                } else {
                    x[j] = xv;
                }
            }
            objective = -sign * L.result[i];
        } else if (status == YALPS_UNBOUNDED) {
            const int32_t *var = L.var + it.perm_off;
            const int at = (int)L.result[i];
            const int v = (unsigned)at < (unsigned)(w + it.h) ? var[at] - 1 : -1;
            if constexpr (BOUNDS) {
                for (int j = tid; j < n; j += T) {
                    const double xv = j == v ? INFINITY : 0.0;
                    x[j] = lb ? xv + lb[(long long)j * lbs] : xv;
                }
            } else {
                for (int j = tid; j < n; j += T) x[j] = j == v ? INFINITY : 0.0;
            }
            objective = sign * INFINITY;
        } else {
            for (int j = tid; j < n; j += T) x[j] = nan; // (NaN + lb[j] is NaN)
        }
        if constexpr (BOUNDS) {
            // (wave 0 alone computes the constant, whole: the condition is the same for all lanes of a wave; the caller's c, not sign * c)
            if (lb && tid < 64) objective = objective + dense_shift_sum(d->c.p + i * d->c.sb, d->c.sr, lb, lbs, n);
        }
        if (tid == 0) d->objective[i] = objective;
        if (d->ineqlin || d->eqlin || d->reduced) dense_marginals<T>(d, L.pos + it.perm_off, mat, i, w, status == YALPS_OPTIMAL);
        if constexpr (BOUNDS) {
            if (d->upper) dense_upper_marginals<T>(d, L.pos + it.perm_off, mat, i, w, status == YALPS_OPTIMAL);
        }
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_dense_kernel(DenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJob<false>(L));
}

// the same queue with bounds; instantiated by lp_dense_bounds.hip alone (libyalps_lpdense_bounds.so)
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_dense_bounds_kernel(DenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseJob<true>(L));
}

// ------------------------------------------------------------------------------------------ free variables
// the effective lower bound of variable j: +0.0 at a free variable, where lb is not read
__device__ __forceinline__ double dense_free_low(const double *l, long long sl, const int32_t *twin, int j) {
    return twin[j] >= 0 ? 0.0 : l[(long long)j * sl];
}

// shift_sum(a, l_eff) over the n original columns, THE order of dense_shift_sum
__device__ __forceinline__ double dense_free_shift_sum(const double *a, long long sa, const double *l, long long sl, const int32_t *twin,
                                                       int n) {
    double p = 0.0;
    for (int j = threadIdx.x & 63; j < n; j += 64) p = p + a[(long long)j * sa] * dense_free_low(l, sl, twin, j);
    for (int s = 32; s > 0; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

// cost_nb(v): cost at the column variable v ended in, 0 where it is basic
__device__ __forceinline__ double dense_cost_nb(const double *mat, const int32_t *pos, int w, int v) {
    const int p = pos[v];
    return p < w ? dense_cost(mat, p) : 0.0;
}

// dense_marginals for a tableau of n + n_free columns: the rows' formulas with the wider w, reduced[n] with the twin's term
template <int T>
__device__ __forceinline__ void dense_free_marginals(const DenseCall *d, const int32_t *pos, const double *mat, long long i, int w,
                                                     bool optimal) {
    const int tid = threadIdx.x, n = d->n, m_ub = d->m_ub, m_eq = d->m_eq;
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
        const int32_t *twin = d->twin;
        for (int j = tid; j < n; j += T) {
            double v = nan;
            if (optimal) {
                const int tj = twin[j];
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
}

// DenseFreeJob::fill.  A function of its own, not inlined, as dense_free_readout and for its reason: with the read-out alone out
// of line the <1024,check> HBM form still spilled two registers.
template <int T>
__device__ __attribute__((noinline)) void dense_free_fill(const DenseCall *d, long long i, int w, int h, double *mat, double *rhs, int32_t *pos,
                                                          int32_t *var, int lp) {
    const int tid = threadIdx.x, n = d->n, nw = w - 1, m_ub = d->m_ub; // nw: the originals and the twins
    const double sign = d->sign;
    const int Uc = wg_unit_lanes(lp + 1, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
    const int32_t *twin = d->twin, *free_idx = d->free_idx;
    const double *lb = nullptr, *ub = nullptr;
    const long long lbs = d->lb.sr, ubs = d->ub.sr;
    const int h0 = h - d->n_upper; // the first bound row
    if (d->lb.p) lb = d->lb.p + i * d->lb.sb;
    if (d->ub.p) ub = d->ub.p + i * d->ub.sb;
    if (lb) { // the shifts: one wave per operand row, parked in the row's rhs slot
        const int m_eq = d->m_eq;
        for (int q = tid >> 6; q < m_ub + m_eq; q += T >> 6) {
            const bool eq = q >= m_ub;
            const DenseOperand &A = eq ? d->A_eq : d->A_ub;
            const int k = eq ? q - m_ub : q;
            const double v = dense_free_shift_sum(A.p + i * A.sb + (long long)k * A.sr, A.sc, lb, lbs, twin, n);
            if ((tid & 63) == 0) {
                if (eq) rhs[1 + m_ub + 2 * k] = rhs[2 + m_ub + 2 * k] = v;
                else rhs[1 + q] = v;
            }
        }
        __syncthreads();
    }
    for (int r = cg0; r < h; r += CG) {
        double *dst = mat + (size_t)r * lp;
        if (r >= h0) { // a bound row: nothing but column 0 is read; -1.0 at the twin of a free variable
            const int j = d->upper_idx[r - h0], tj = twin[j] - 1;
            for (int c = cu0; c <= lp; c += Uc) {
                if (c == lp) {
                    const double u = ub[(long long)j * ubs];
                    rhs[r] = lb ? u - dense_free_low(lb, lbs, twin, j) : u;
                } else {
                    dst[c] = c == j ? 1.0 : (c == tj ? -1.0 : 0.0);
                }
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
                if (lb && r != 0) {
                    const double v = *b - rhs[r];
                    rhs[r] = neg ? -v : v;
                } else {
                    rhs[r] = r == 0 ? 0.0 : (neg ? -*b : *b);
                }
            } else if (c >= nw) {
                dst[c] = 0.0;
            } else { // column c of the originals, or the twin of free_idx[c - n]: the negation of the cell written there
                const bool tw = c >= n;
                const double v = a[(long long)(tw ? free_idx[c - n] : c) * sc];
                const double cell = r == 0 ? sign * v : (neg ? -v : v);
                dst[c] = tw ? -cell : cell;
            }
        }
    }
    for (int p = tid; p < w + h; p += T) {
        pos[p] = p;
        var[p] = p;
    }
}

// DenseFreeJob::after behind its barrier: solution() on the device with x[j] = v(p) - v(q) at a free variable, and the marginals.
// A function of its own, not inlined (as lp_sens_kernel's epilogue and for its reason): inlined, its registers came on top of
// wg_simplex's in the allocator's eyes and the <1024,check> HBM form spilled two registers to scratch.
template <int T>
__device__ __attribute__((noinline)) void dense_free_readout(const DenseCall *d, const int32_t *pos, const int32_t *var, const double *result,
                                                             const double *mat, const double *rhs, long long i, int w, int h, int status) {
    const int tid = threadIdx.x, n = d->n;
    double *x = d->x + i * n;
    const double sign = d->sign, p = d->precision;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    const int32_t *twin = d->twin;
    double objective = nan;
    const double *lb = nullptr; // x = x' + l_eff, whatever the status
    const long long lbs = d->lb.sr;
    if (d->lb.p) lb = d->lb.p + i * d->lb.sb;
    if (status == YALPS_OPTIMAL) {
        for (int j = tid; j < n; j += T) {
            const int row = pos[j + 1] - w, tj = twin[j];
            const double v = row >= 0 ? rhs[row] : 0.0;
            double xv = v > p ? round_to_precision(v, p) : 0.0;
            if (tj >= 0) {
                const int qrow = pos[tj] - w;
                const double q = qrow >= 0 ? rhs[qrow] : 0.0;
                xv = xv - (q > p ? round_to_precision(q, p) : 0.0);
            }
            x[j] = lb ? xv + (tj >= 0 ? 0.0 : lb[(long long)j * lbs]) : xv;
        }
        objective = -sign * *result;
    } else if (status == YALPS_UNBOUNDED) {
        const int at = (int)*result;
        const int v = (unsigned)at < (unsigned)(w + h) ? var[at] : -1; // the unbounded column, 1-based
        for (int j = tid; j < n; j += T) {
            const int tj = twin[j];
            double xv = j + 1 == v ? INFINITY : 0.0;
            if (tj >= 0) xv = xv - (tj == v ? INFINITY : 0.0);
            x[j] = lb ? xv + (tj >= 0 ? 0.0 : lb[(long long)j * lbs]) : xv;
        }
        objective = sign * INFINITY;
    } else {
        for (int j = tid; j < n; j += T) x[j] = nan; // (NaN + l_eff[j] is NaN)
    }
    // (wave 0 alone computes the constant, whole: the condition is the same for all lanes of a wave; the caller's c, not sign * c)
    if (lb && tid < 64) objective = objective + dense_free_shift_sum(d->c.p + i * d->c.sb, d->c.sr, lb, lbs, twin, n);
    if (tid == 0) d->objective[i] = objective;
    if (d->ineqlin || d->eqlin || d->reduced) dense_free_marginals<T>(d, pos, mat, i, w, status == YALPS_OPTIMAL);
    if (d->upper) dense_upper_marginals<T>(d, pos, mat, i, w, status == YALPS_OPTIMAL);
}

// DenseJob<true> with n_free twin columns; lb / ub may be absent (null descriptors), as there
struct DenseFreeJob : QueueJobBase {
    const DenseLaunch &L;
    const DenseCall *d;
    int idx;
    __device__ __forceinline__ explicit DenseFreeJob(const DenseLaunch &launch) : L(launch), d(launch.call), idx(0) {}
    __device__ __forceinline__ QueueItem item(int i) {
        idx = i;
        const int w = d->n + 1 + d->n_free, h = 1 + d->m_ub + 2 * d->m_eq + d->n_upper, heven = (h + 1) & ~1;
        return QueueItem{w, h, (long long)((size_t)i * heven), (long long)((size_t)i * ((size_t)w + h)), d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int i, const QueueItem &it) const { return (long long)((size_t)i * it.w * it.h); }

    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        dense_free_fill<T>(d, idx, it.w, it.h, mat, rhs, pos, var, lp);
    }

    // solution() on the device: dense_free_readout.  Every lane; the barrier is met whatever the status.
    template <int T>
    __device__ __forceinline__ void after(const QueueItem &it, int status, const double *mat, const double *rhs, int) const {
        __syncthreads(); // the queue's copies of pos / var / col0 and lane T - 1's result are written
        if (status == WG_HISTORY_FULL) return;
        dense_free_readout<T>(d, L.pos + it.perm_off, L.var + it.perm_off, L.result + idx, mat, rhs, idx, it.w, it.h, status);
    }
};

// the same queue with free variables; instantiated by lp_dense_free.hip alone (libyalps_lpdense_free.so)
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_dense_free_kernel(DenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, DenseFreeJob(L));
}
