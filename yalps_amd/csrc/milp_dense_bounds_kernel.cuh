// milp_dense_bounds_kernel.cuh -- milp_dense_kernel.cuh's two kernels for a call with variable bounds lb <= x <= ub: the root
// LPs with the bound rows and the shifted right-hand sides, and solution() moved back to x.  Instantiated by
// milp_dense_bounds.hip alone (libyalps_milpdense_bounds.so); milp_dense.hip includes this file for the two structs, inside its
// anonymous namespace, behind milp_dense_kernel.cuh and lp_dense_kernel.cuh's order of summation, which is restated here.
#pragma once
#include "milp_dense_kernel.cuh"

// ------------------------------------------------------------------------------------------
// x >= lb replaces x >= 0 by the substitution x = l_eff + x', and x[j] <= ub[j] for the n_upper listed variables adds n_upper
// rows between the equality rows and the binary rows: h0 = 1 + m_ub + 2 * m_eq, h = h0 + n_upper + n_bin.
//   l_eff[j]  by the column's kind byte: 0 continuous lb[j]; 1 integer ceil(lb[j]) (IEEE: ceil(-0.5) is -0.0, NaN and the
//          infinities pass through), so that x' is integral where x is and milp_tree_kernel branches on x' knowing nothing of
//          bounds; 2 binary +0.0, lb is not read there.  Kinds, `upper_idx` and `bin` are host decisions, uploaded behind the
//          call's description.
//   shift_sum(a, l_eff), THE order of lp_dense_kernel.cuh: every product a[j] * l_eff[j] rounded on its own (with +0.0 at a
//          binary column too: a coefficient that is not finite gives NaN there); lane k of ONE wave adds the products of the
//          columns j = k (mod 64) in ascending j to +0.0; then p += shfl_down(p, s) for s = 32, 16, 8, 4, 2, 1; lane 0 holds it.
//   fill   MilpDenseJob::fill plus three parts.  With lb: a pass in front of the row loop, one wave per operand row, parks
//          the row's shift_sum in the row's rhs slot (both slots of an equality); one barrier; the row loop's column-0 lane
//          then writes b - rhs[r], one subtraction (its negation in the second row of an equality).  Bound row t, between the
//          equality rows and the binary rows: ub[j] - l_eff[j] (or ub[j]) in column 0, 1.0 in column j = upper_idx[t], else
//          +0.0: generated, not read.  No binary variable is listed, so ub is not read at one.  Binary rows as before.
//   no `after`: the tableaux are kept for the trees, x is written by milp_dense_bounds_solution_kernel.
// Every branch on "has lb" and on the row's kind is the workgroup's or the group's of lanes that share a row; the column's
// kind of a bound row is read by the one lane that writes column 0.
// ------------------------------------------------------------------------------------------
struct MilpDenseBoundsCall : MilpDenseCall { // (behind every field the boundless kernels read)
    MilpDenseOperand lb, ub;      // (batch, row) = (i, j), sc unused; p = nullptr: absent
    int32_t n_upper, pad2_;       // bound rows; ub is read at upper_idx[0 .. n_upper) only
    const int32_t *upper_idx;     // device, ascending, no binary variable in it
    const uint8_t *kind;          // [n] 0 continuous, 1 integer, 2 binary
};

// l_eff[j]; l = nullptr never gets here
__device__ __forceinline__ double milp_l_eff(const double *l, long long sl, const uint8_t *kind, int j) {
    const int k = kind[j];
    if (k == 2) return 0.0;
    const double v = l[(long long)j * sl];
    return k == 1 ? ceil(v) : v;
}

// shift_sum(a, l_eff) over n columns in the canonical order: every lane of a wave calls it, lane 0's value is the sum
__device__ __forceinline__ double milp_shift_sum(const double *a, long long sa, const double *l, long long sl, const uint8_t *kind, int n) {
    double p = 0.0;
    for (int j = threadIdx.x & 63; j < n; j += 64) p = p + a[(long long)j * sa] * milp_l_eff(l, sl, kind, j);
    for (int s = 32; s > 0; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

struct MilpDenseBoundsJob : QueueJobBase {
    const MilpDenseBoundsCall *d;
    int idx;
    __device__ __forceinline__ explicit MilpDenseBoundsJob(const MilpDenseLaunch &launch)
        : d(static_cast<const MilpDenseBoundsCall *>(launch.call)), idx(0) {}
    __device__ __forceinline__ QueueItem item(int i) {
        idx = i;
        const int w = d->n + 1, h = 1 + d->m_ub + 2 * d->m_eq + d->n_upper + d->n_bin, heven = (h + 1) & ~1;
        return QueueItem{w, h, (long long)((size_t)i * heven), (long long)((size_t)i * ((size_t)w + h)), d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int i, const QueueItem &it) const { return (long long)((size_t)i * it.w * it.h); }

    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        const int tid = threadIdx.x, w = it.w, h = it.h, n = w - 1, m_ub = d->m_ub, m_eq = d->m_eq;
        const int h0 = 1 + m_ub + 2 * m_eq, hb = h - d->n_bin; // the first bound row, the first binary row
        const long long i = idx;
        const double sign = d->sign;
        // a group of Uc lanes per row, the lanes along its columns (lane `lp` of a row, where it exists, writes column 0)
        const int Uc = wg_unit_lanes(lp + 1, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
        const long long lbs = d->lb.sr, ubs = d->ub.sr;
        const double *lb = d->lb.p ? d->lb.p + i * d->lb.sb : nullptr;
        const double *ub = d->ub.p ? d->ub.p + i * d->ub.sb : nullptr;
        const uint8_t *kind = d->kind;
        if (lb) { // the shifts: one wave per operand row, parked in the row's rhs slot
            for (int q = tid >> 6; q < m_ub + m_eq; q += T >> 6) {
                const bool eq = q >= m_ub;
                const MilpDenseOperand &A = eq ? d->A_eq : d->A_ub;
                const int k = eq ? q - m_ub : q;
                const double v = milp_shift_sum(A.p + i * A.sb + (long long)k * A.sr, A.sc, lb, lbs, kind, n);
                if ((tid & 63) == 0) {
                    if (eq) rhs[1 + m_ub + 2 * k] = rhs[2 + m_ub + 2 * k] = v;
                    else rhs[1 + q] = v;
                }
            }
            __syncthreads();
        }
        for (int r = cg0; r < h; r += CG) {
            double *dst = mat + (size_t)r * lp;
            if (r >= h0) { // a generated row (r is the same for the lanes of a group): nothing but column 0 is read
                const bool binary = r >= hb; // x <= 1, or x' <= ub - l_eff
                const int j = binary ? d->bin[r - hb] : d->upper_idx[r - h0];
                for (int c = cu0; c <= lp; c += Uc) {
                    if (c == lp) {
                        double v = 1.0;
                        if (!binary) {
                            const double u = ub[(long long)j * ubs];
                            v = lb ? u - milp_l_eff(lb, lbs, kind, j) : u;
                        }
                        rhs[r] = v;
                    } else {
                        dst[c] = c == j ? 1.0 : 0.0;
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
__global__ __launch_bounds__(T) void milp_dense_bounds_root_kernel(MilpDenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, MilpDenseBoundsJob(L));
}

// ------------------------------------------------------------------------------------------
// milp_dense_bounds_solution_kernel: milp_dense_solution_kernel, then x[j] = x'[j] + l_eff[j] -- one addition per element
// whatever the status (NaN + l_eff is NaN) -- and objective = objective' + shift_sum(c, l_eff), one addition after the
// rounding: wave 0 recomputes the sum alone and whole from the caller's c (not sign * c), lane 0 adds and writes it, as
// DenseJob<true>::after does.  Without lb nothing is added.  Plain stores.
// ------------------------------------------------------------------------------------------
struct MilpBoundsSolutionArgs : MilpSolutionArgs {
    MilpDenseOperand c, lb;       // lb.p = nullptr: absent
    const uint8_t *kind;          // [n]
};

template <int T>
__global__ __launch_bounds__(T) void milp_dense_bounds_solution_kernel(MilpBoundsSolutionArgs a) {
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
    const long long lbs = a.lb.sr;
    const double *lb = a.lb.p ? a.lb.p + (long long)i * a.lb.sb : nullptr;
    const uint8_t *kind = a.kind;
    double *x = a.x ? a.x + i * (size_t)n : nullptr;
    double objective = nan;
    if (st == YALPS_OPTIMAL || (st == MT_TIMEDOUT && has)) {
        if (x)
            for (int j = tid; j < n; j += T) {
                const int row = pos[j + 1] - w;
                const double v = (unsigned)row < (unsigned)h ? col0[row] : 0.0;
                const double xv = v > p ? round_to_precision(v, p) : 0.0;
                x[j] = lb ? xv + milp_l_eff(lb, lbs, kind, j) : xv;
            }
        objective = -sign * res;
    } else if (st == YALPS_UNBOUNDED) {
        const int at = (int)res;
        const int v = (unsigned)at < (unsigned)(w + h) ? var[at] - 1 : -1;
        if (x)
            for (int j = tid; j < n; j += T) {
                const double xv = j == v ? INFINITY : 0.0;
                x[j] = lb ? xv + milp_l_eff(lb, lbs, kind, j) : xv;
            }
        objective = sign * INFINITY;
    } else {
        if (x)
            for (int j = tid; j < n; j += T) x[j] = nan; // (NaN + l_eff[j] is NaN)
    }
    // (wave 0 alone computes the constant, whole: the condition is the same for all lanes of a wave)
    if (lb && tid < 64) objective = objective + milp_shift_sum(a.c.p + (long long)i * a.c.sb, a.c.sr, lb, lbs, kind, n);
    if (tid == 0) {
        if (a.objective) a.objective[i] = objective;
        if (st < 0 || st > MT_TIMEDOUT) {
            if (a.status_out) a.status_out[i] = a.overflow;
            if (a.nodes_out) a.nodes_out[i] = 0;
            if (a.node_pivots_out) a.node_pivots_out[i] = 0;
        }
    }
}
