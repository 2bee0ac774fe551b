// milp_dense_free_kernel.cuh -- milp_dense_bounds_kernel.cuh's two kernels for a call with free variables: the root LPs with one
// twin column per free variable behind the n originals, and solution() read off the wider tableau with the halves subtracted.
// Instantiated by milp_dense_free.hip alone (libyalps_milpdense_free.so); milp_dense.hip includes this file for the two structs,
// inside its anonymous namespace, behind milp_dense_bounds_kernel.cuh.
#pragma once
#include "milp_dense_bounds_kernel.cuh"

// ------------------------------------------------------------------------------------------
// A free variable j is split as x[j] = p[j] - q[j], p, q >= 0, by lp_dense_kernel.cuh's rules (DenseFreeJob): p keeps column
// 1 + j, the twins q are n_free generated columns behind the n originals in ascending j: w = 1 + n + n_free,
// h0 = 1 + m_ub + 2 * m_eq, h = h0 + n_upper + n_bin.
//   l_eff[j]  +0.0 at a free variable, integer or not: lb is not read there and nothing is ceiled; else milp_l_eff's (lb,
//          ceil(lb) at an integer variable, +0.0 at a binary one).  No binary variable is free (a host refusal).
//   shift_sum(a, l_eff) over the n original columns alone, THE order of lp_dense_kernel.cuh; the product with the +0.0 of a
//          free variable is still formed and added.
//   fill   MilpDenseBoundsJob::fill, and for column c >= 1 + n of an operand row the IEEE negation of the cell written at the
//          column of free_idx[c - 1 - n] in that row -- of the value written there, not a second product: one strided read of
//          the operand by the lane that owns the column.  Bound row of a free variable: -1.0 in the twin's column; every other
//          generated row, the binary rows included: +0.0 there.  lb and ub may both be absent.
//   no `after`: the tableaux are kept for the trees.  milp_tree_kernel branches on the integer columns it is given: the host
//          lists the twin of a free integer variable behind the n_int columns 1 + j, so that q is integral where p is.
// Every branch is on "has lb" (the workgroup's), on the row's kind (a group of lanes that share a row) or on the column (a lane);
// none is per MILP.
// ------------------------------------------------------------------------------------------
struct MilpDenseFreeCall : MilpDenseBoundsCall { // (behind every field the boundless and the bounded kernels read)
    int32_t n_free, pad3_;        // twin columns behind the n originals
    const int32_t *free_idx;      // device, ascending: twin t (column 1 + n + t) is the twin of variable free_idx[t]
    const int32_t *twin;          // device, [n]: the twin's column 1 + n + t of a free variable, -1 of any other
};

// l_eff[j]; l = nullptr never gets here
__device__ __forceinline__ double milp_free_l_eff(const double *l, long long sl, const uint8_t *kind, const int32_t *twin, int j) {
    return twin[j] >= 0 ? 0.0 : milp_l_eff(l, sl, kind, j);
}

// shift_sum(a, l_eff) over the n original columns in the canonical order: every lane of a wave calls it, lane 0's value is the sum
__device__ __forceinline__ double milp_free_shift_sum(const double *a, long long sa, const double *l, long long sl, const uint8_t *kind,
                                                      const int32_t *twin, int n) {
    double p = 0.0;
    for (int j = threadIdx.x & 63; j < n; j += 64) p = p + a[(long long)j * sa] * milp_free_l_eff(l, sl, kind, twin, j);
    for (int s = 32; s > 0; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

// MilpDenseFreeJob::fill.  Inlined, unlike dense_free_fill (lp_dense_kernel.cuh): this job has no `after`, so the <1024,check>
// HBM form keeps 7 registers to spare (121 of 128, no scratch), while as a noinline function the fill itself spilled 36 bytes
// in all four 1024-lane forms -- a callee cannot borrow the registers its caller has free.
template <int T>
__device__ __forceinline__ void milp_dense_free_fill(const MilpDenseFreeCall *d, long long i, int w, int h, double *mat, double *rhs,
                                                     int32_t *pos, int32_t *var, int lp) {
    const int tid = threadIdx.x, n = d->n, nw = w - 1, m_ub = d->m_ub, m_eq = d->m_eq; // nw: the originals and the twins
    const int h0 = 1 + m_ub + 2 * m_eq, hb = h - d->n_bin; // the first bound row, the first binary row
    const double sign = d->sign;
    // a group of Uc lanes per row, the lanes along its columns (lane `lp` of a row, where it exists, writes column 0)
    const int Uc = wg_unit_lanes(lp + 1, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
    const long long lbs = d->lb.sr, ubs = d->ub.sr;
    const double *lb = d->lb.p ? d->lb.p + i * d->lb.sb : nullptr;
    const double *ub = d->ub.p ? d->ub.p + i * d->ub.sb : nullptr;
    const uint8_t *kind = d->kind;
    const int32_t *twin = d->twin, *free_idx = d->free_idx;
    if (lb) { // the shifts: one wave per operand row, parked in the row's rhs slot
        for (int q = tid >> 6; q < m_ub + m_eq; q += T >> 6) {
            const bool eq = q >= m_ub;
            const MilpDenseOperand &A = eq ? d->A_eq : d->A_ub;
            const int k = eq ? q - m_ub : q;
            const double v = milp_free_shift_sum(A.p + i * A.sb + (long long)k * A.sr, A.sc, lb, lbs, kind, twin, n);
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
            const bool binary = r >= hb; // x <= 1, or x' <= ub - l_eff with -1.0 at the twin of a free variable
            const int j = binary ? d->bin[r - hb] : d->upper_idx[r - h0];
            const int tj = binary ? -1 : twin[j] - 1; // (a variable without a twin: -2, no column)
            for (int c = cu0; c <= lp; c += Uc) {
                if (c == lp) {
                    double v = 1.0;
                    if (!binary) {
                        const double u = ub[(long long)j * ubs];
                        v = lb ? u - milp_free_l_eff(lb, lbs, kind, twin, j) : u;
                    }
                    rhs[r] = v;
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

struct MilpDenseFreeJob : QueueJobBase {
    const MilpDenseFreeCall *d;
    int idx;
    __device__ __forceinline__ explicit MilpDenseFreeJob(const MilpDenseLaunch &launch)
        : d(static_cast<const MilpDenseFreeCall *>(launch.call)), idx(0) {}
    __device__ __forceinline__ QueueItem item(int i) {
        idx = i;
        const int w = d->n + 1 + d->n_free, h = 1 + d->m_ub + 2 * d->m_eq + d->n_upper + d->n_bin, heven = (h + 1) & ~1;
        return QueueItem{w, h, (long long)((size_t)i * heven), (long long)((size_t)i * ((size_t)w + h)), d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int i, const QueueItem &it) const { return (long long)((size_t)i * it.w * it.h); }

    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        milp_dense_free_fill<T>(d, idx, it.w, it.h, mat, rhs, pos, var, lp);
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_dense_free_root_kernel(MilpDenseLaunch L) {
    wg_queue<T, CHECK, LDS>(L, MilpDenseFreeJob(L));
}

// ------------------------------------------------------------------------------------------
// milp_dense_free_solution_kernel: milp_dense_bounds_solution_kernel on the best tableau of width w = 1 + n + n_free, with
// dense_free_readout's rule (lp_dense_kernel.cuh) at a free variable j, whose twin's column is twin[j]:
//   "optimal", "timedout" with a result: x[j] = v(p) - v(q), each v solution()'s rule on its own column (basic and above
//       precision: rounded; anything else +0.0), one subtraction; then + l_eff[j] where lb is given
//   "unbounded": +inf at the unbounded column, so -inf where that column is a twin
//   anything else: NaN
// objective = objective' + shift_sum(c, l_eff) over the n originals, one addition, by wave 0 from the caller's c.  The lane that
// owns j reads twin[j] and, for a free variable, one more pos entry: no barrier, no LDS.  Plain stores.
// ------------------------------------------------------------------------------------------
struct MilpFreeSolutionArgs : MilpBoundsSolutionArgs {
    int32_t n_free, pad_;
    const int32_t *twin;          // [n]
};

template <int T>
__global__ __launch_bounds__(T) void milp_dense_free_solution_kernel(MilpFreeSolutionArgs a) {
    const int tid = threadIdx.x, n = a.n, w = n + 1 + a.n_free;
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
    const int32_t *twin = a.twin;
    double *x = a.x ? a.x + i * (size_t)n : nullptr;
    double objective = nan;
    if (st == YALPS_OPTIMAL || (st == MT_TIMEDOUT && has)) {
        if (x)
            for (int j = tid; j < n; j += T) {
                const int row = pos[j + 1] - w, tj = twin[j];
                const double v = (unsigned)row < (unsigned)h ? col0[row] : 0.0;
                double xv = v > p ? round_to_precision(v, p) : 0.0;
                if (tj >= 0) {
                    const int qrow = pos[tj] - w;
                    const double q = (unsigned)qrow < (unsigned)h ? col0[qrow] : 0.0;
                    xv = xv - (q > p ? round_to_precision(q, p) : 0.0);
                }
                x[j] = lb ? xv + milp_free_l_eff(lb, lbs, kind, twin, j) : xv;
            }
        objective = -sign * res;
    } else if (st == YALPS_UNBOUNDED) {
        const int at = (int)res;
        const int v = (unsigned)at < (unsigned)(w + h) ? var[at] : -1; // the unbounded column, 1-based
        if (x)
            for (int j = tid; j < n; j += T) {
                const int tj = twin[j];
                double xv = j + 1 == v ? INFINITY : 0.0;
                if (tj >= 0) xv = xv - (tj == v ? INFINITY : 0.0);
                x[j] = lb ? xv + milp_free_l_eff(lb, lbs, kind, twin, j) : xv;
            }
        objective = sign * INFINITY;
    } else {
        if (x)
            for (int j = tid; j < n; j += T) x[j] = nan; // (NaN + l_eff[j] is NaN)
    }
    // (wave 0 alone computes the constant, whole: the condition is the same for all lanes of a wave)
    if (lb && tid < 64) objective = objective + milp_free_shift_sum(a.c.p + (long long)i * a.c.sb, a.c.sr, lb, lbs, kind, twin, n);
    if (tid == 0) {
        if (a.objective) a.objective[i] = objective;
        if (st < 0 || st > MT_TIMEDOUT) {
            if (a.status_out) a.status_out[i] = a.overflow;
            if (a.nodes_out) a.nodes_out[i] = 0;
            if (a.node_pivots_out) a.node_pivots_out[i] = 0;
        }
    }
}
