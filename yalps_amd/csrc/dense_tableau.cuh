// dense_tableau.cuh -- the dense tableau of the tensor solvers, each rule once: the description of a call, the initial tableau
// built from strided device operands (fill), solution() read off the final one (read-out), and the LP marginals.
// Included by lp_dense_kernel.cuh and milp_dense_kernel.cuh inside their libraries' anonymous namespaces (gfx950 only); the six
// families -- linprog_batch and milp_batch, each plain, with bounds, with free variables -- are DenseTraits of the code below.
#pragma once
#include "wg_queue.cuh"

// ------------------------------------------------------------------------------------------
// All problems of a call share one shape: n variables, m_ub rows A_ub x <= b_ub, m_eq rows A_eq x = b_eq.  The tableau
// (tableauModel's, src/tableau.ts:47-137) has w = 1 + n + n_free columns and h = h0 + n_upper + n_bin rows, h0 = 1 + m_ub + 2 * m_eq:
//   row 0                 +0.0, sign * c[j] (a product: -1 * 0.0 is -0.0)
//   row 1 + i             b_ub[i], A_ub[i, j]
//   rows 1 + m_ub + 2k, and the one after it: b_eq[k], A_eq[k, j] and their IEEE negations (a zero becomes -0.0)
//   row h0 + t            (bounds) the bound row of variable j = upper_idx[t]: ub[j] - l_eff[j] (or ub[j]) in column 0, 1.0 in
//                         column j, -1.0 in the twin's column of a free variable, else +0.0: generated, not read
//   row h0 + n_upper + q  (MILP) the row of the q-th binary variable j = bin[q], x <= 1 (src/tableau.ts:122-128): 1.0 in
//                         column 0 and in column j, else +0.0.  No binary variable has a bound row or a twin (host refusals).
// Identity permutations; the padding columns of the pitch +0.0.  Values are taken as they lie in memory: a NaN or an infinity
// goes into the tableau.  Lanes run along the columns of a row, so an operand whose column stride is 1 is read coalesced.
//
// Bounds: x >= lb replaces x >= 0 by the substitution x = l_eff + x'.
//   l_eff[j]   lb[j]; (MILP, by the column's kind byte) ceil(lb[j]) at an integer variable -- IEEE: ceil(-0.5) is -0.0, NaN and
//          the infinities pass through -- so that x' is integral where x is and milp_tree_kernel branches on x' knowing nothing
//          of bounds, and +0.0 at a binary one, where lb is not read; (free) +0.0 at a free variable, integer or not, where
//          lb is not read and nothing is ceiled.
//   shift_sum(a, l_eff), THE order: every product a[j] * l_eff[j] rounded on its own (the product with a +0.0 is still formed:
//          a coefficient that is not finite gives NaN there); lane k of ONE wave adds the products of the columns j = k (mod 64)
//          in ascending j to +0.0; then p += shfl_down(p, s) for s = 32, 16, 8, 4, 2, 1; lane 0 holds it.  It runs over the n
//          original columns alone and depends on nothing but a and l_eff: not on T, the LDS / HBM / aux form, strides or the batch.
//   fill   with lb: a pass in front of the row loop, one wave per operand row, parks the row's shift_sum in the row's rhs slot
//          (both slots of an equality); one barrier; the row loop's column-0 lane then writes b - rhs[r], one subtraction (its
//          negation in the second row of an equality).  Without lb nothing is subtracted.  Coefficients and row 0 are untouched.
// Free variables: x[j] = p[j] - q[j], p, q >= 0.  p keeps column 1 + j, the twins q are n_free generated columns behind the n
// originals in ascending j.  A twin cell of an operand row is the IEEE negation of the cell of column 1 + j in the same row -- of
// the value written there, not a second product: one strided read of the operand at free_idx[c - n] by the lane that owns column c.
// Every branch is on "has lb" (the workgroup's), on the row's group (lanes that share a row) or on the column (a lane), never
// per problem.
//
// The call's description lies in device memory, not in the kernel's arguments: five operands with three 64-bit strides each
// would sit in scalar registers through the solve.  A kernel reads the fields of its family alone (below), and the host
// uploads no more than those.
// ------------------------------------------------------------------------------------------
struct DenseOperand {
    const double *p;              // element (i, r, c) at p[i * sb + r * sr + c * sc]; a vector has sc = 0 and is indexed by r
    long long sb, sr, sc;
};

struct DenseDesc {
    int32_t n, m_ub, m_eq, aux_hbm; // aux_hbm: HBM form, colbuf / prow behind the tableau in the workspace
    double sign;                  // +1 maximise, -1 minimise
    double precision, max_pivots;
    DenseOperand c, A_ub, b_ub, A_eq, b_eq; // c and the b's: (batch, row) = (i, j), sc unused
    int32_t n_bin, n_upper, n_free, pad_; // binary rows (MILP), bound rows, twin columns: 0 in a family without them
    const int32_t *bin;           // device, [n_bin] 0-based variable indices, ascending
    // ---- with bounds and with free variables (a plain kernel reads nothing from here on)
    DenseOperand lb, ub;          // (batch, row) = (i, j), sc unused; p = nullptr: absent.  ub is read at upper_idx[0 .. n_upper) only
    const int32_t *upper_idx;     // device, ascending, no binary variable in it
    const uint8_t *kind;          // device, [n] 0 continuous, 1 integer, 2 binary (MILP)
    // ---- with free variables
    const int32_t *free_idx;      // device, ascending: twin t (column 1 + n + t) is the twin of variable free_idx[t]
    const int32_t *twin;          // device, [n]: the twin's column 1 + n + t of a free variable, -1 of any other
};
// the bytes of it a family's kernels read
constexpr size_t dense_desc_bytes(bool bounds, bool free) {
    return free ? sizeof(DenseDesc) : bounds ? offsetof(DenseDesc, free_idx) : offsetof(DenseDesc, lb);
}

// A family: which of the generated parts its kernels hold.  `if constexpr` on these, so a plain kernel contains no instruction
// of the others.  (free implies bounds: the free kernels take lb / ub, which may both be absent.)
template <bool BOUNDS, bool FREE, bool MILP>
struct DenseTraits {
    static constexpr bool bounds = BOUNDS, free = FREE, milp = MILP;
    static_assert(BOUNDS || !FREE, "the free kernels are the bounded ones plus the twins");
};

// l_eff of one problem: its lb row (l = nullptr: the call has none, and at() is not called) and the call's kind bytes / twins
struct DenseLow {
    const double *l;
    long long sl;
    const uint8_t *kind;
    const int32_t *twin;
    template <class F>
    __device__ __forceinline__ double at(int j) const {
        if constexpr (F::free)
            if (twin[j] >= 0) return 0.0;
        if constexpr (F::milp) {
            const int k = kind[j];
            if (k == 2) return 0.0;
            const double v = l[(long long)j * sl];
            return k == 1 ? ceil(v) : v;
        } else {
            return l[(long long)j * sl];
        }
    }
};
// of problem i, from what names lb, kind and twin (a DenseDesc, or the MILP epilogue's arguments): its family's fields alone are read
template <class F, class From>
__device__ __forceinline__ DenseLow dense_low(const From &s, long long i) {
    DenseLow low{s.lb.p ? s.lb.p + i * s.lb.sb : nullptr, s.lb.sr, nullptr, nullptr};
    if constexpr (F::milp) low.kind = s.kind;
    if constexpr (F::free) low.twin = s.twin;
    return low;
}

// shift_sum(a, l_eff) over n columns in THE order (above): every lane of a wave calls it, lane 0's value is the sum
template <class F>
__device__ __forceinline__ double dense_shift_sum(const double *a, long long sa, const DenseLow &low, int n) {
    double p = 0.0;
    for (int j = threadIdx.x & 63; j < n; j += 64) p = p + a[(long long)j * sa] * low.at<F>(j);
    for (int s = 32; s > 0; s >>= 1) p = p + __shfl_down(p, s, 64);
    return p;
}

// where operand row r < h0 of problem i lies: its coefficients, their stride, its right-hand side (row 0: none), negated or not
struct DenseRow {
    const double *a, *b;
    long long sc;
    bool neg;
};
__device__ __forceinline__ DenseRow dense_row(const DenseDesc *d, long long i, int r, int m_ub) {
    if (r == 0) return DenseRow{d->c.p + i * d->c.sb, nullptr, d->c.sr, false};
    if (r <= m_ub)
        return DenseRow{d->A_ub.p + i * d->A_ub.sb + (long long)(r - 1) * d->A_ub.sr, d->b_ub.p + i * d->b_ub.sb + (long long)(r - 1) * d->b_ub.sr,
                        d->A_ub.sc, false};
    const int k = (r - 1 - m_ub) >> 1;
    return DenseRow{d->A_eq.p + i * d->A_eq.sb + (long long)k * d->A_eq.sr, d->b_eq.p + i * d->b_eq.sb + (long long)k * d->b_eq.sr, d->A_eq.sc,
                    ((r - 1 - m_ub) & 1) != 0};
}

// The initial tableau and the permutations of problem i (above).  Every lane; one barrier of its own where the call has lb.
template <int T, class F>
__device__ __forceinline__ void dense_fill(const DenseDesc *d, long long i, int w, int h, double *mat, double *rhs, int32_t *pos, int32_t *var,
                                           int lp) {
    const int tid = threadIdx.x, nw = w - 1, n = F::free ? d->n : nw, m_ub = d->m_ub; // nw: the originals and the twins
    const double sign = d->sign;
    // a group of Uc lanes per row, the lanes along its columns (lane `lp` of a row, where it exists, writes column 0)
    const int Uc = wg_unit_lanes(lp + 1, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
    int hb = h, h0 = h; // the first binary row, the first bound row
    if constexpr (F::milp) h0 = hb = h - d->n_bin;
    DenseLow low{};
    const double *ub = nullptr;
    long long ubs = 0;
    if constexpr (F::bounds) {
        h0 = hb - d->n_upper;
        low = dense_low<F>(*d, i);
        ubs = d->ub.sr;
        if (d->ub.p) ub = d->ub.p + i * d->ub.sb;
        if (low.l) { // the shifts: one wave per operand row, parked in the row's rhs slot
            const int m_eq = d->m_eq;
            for (int q = tid >> 6; q < m_ub + m_eq; q += T >> 6) {
                const bool eq = q >= m_ub;
                const DenseOperand &A = eq ? d->A_eq : d->A_ub;
                const int k = eq ? q - m_ub : q;
                const double v = dense_shift_sum<F>(A.p + i * A.sb + (long long)k * A.sr, A.sc, low, n);
                if ((tid & 63) == 0) {
                    if (eq) rhs[1 + m_ub + 2 * k] = rhs[2 + m_ub + 2 * k] = v;
                    else rhs[1 + q] = v;
                }
            }
            __syncthreads();
        }
    }
    for (int r = cg0; r < h; r += CG) {
        double *dst = mat + (size_t)r * lp;
        if constexpr (F::bounds || F::milp) {
            if (r >= h0) { // a generated row (r is the same for the lanes of a group): nothing but column 0 is read
                const bool binary = F::milp && r >= hb; // x <= 1, or x' <= ub - l_eff
                int j, tj = -1; // the row's variable, the cell of its twin (none: no column)
                if (binary) {
                    j = d->bin[r - hb];
                } else {
                    j = d->upper_idx[r - h0];
                    if constexpr (F::free) tj = low.twin[j] - 1;
                }
                for (int c = cu0; c <= lp; c += Uc) {
                    if (c == lp) {
                        double v = 1.0;
                        if (!binary) {
                            const double u = ub[(long long)j * ubs];
                            v = low.l ? u - low.at<F>(j) : u;
                        }
                        rhs[r] = v;
                    } else {
                        dst[c] = c == j ? 1.0 : (F::free && c == tj ? -1.0 : 0.0);
                    }
                }
                continue;
            }
        }
        const DenseRow row = dense_row(d, i, r, m_ub);
        const bool neg = row.neg;
        for (int c = cu0; c <= lp; c += Uc) {
            if (c == lp) {
                if (F::bounds && low.l && r != 0) {
                    const double v = *row.b - rhs[r];
                    rhs[r] = neg ? -v : v;
                } else {
                    rhs[r] = r == 0 ? 0.0 : (neg ? -*row.b : *row.b);
                }
            } else if (c >= nw) {
                dst[c] = 0.0;
            } else { // column c of the originals, or the twin of free_idx[c - n]: the negation of the cell written there
                const bool tw = F::free && c >= n;
                const double v = row.a[(long long)(tw ? d->free_idx[c - n] : c) * row.sc];
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
// (out of line, for the one job whose registers ask for it: a callee's registers do not come on top of wg_simplex's in the
// allocator's eyes -- and it cannot borrow those its caller has free)
template <int T, class F>
__device__ __attribute__((noinline)) void dense_fill_call(const DenseDesc *d, long long i, int w, int h, double *mat, double *rhs, int32_t *pos,
                                                          int32_t *var, int lp) {
    dense_fill<T, F>(d, i, w, h, mat, rhs, pos, var, lp);
}

// What every dense job tells the queue, and its first step.  OUTLINE: fill (and an LP job's read-out) as calls.
template <class F, bool OUTLINE = false>
struct DenseJobBase : QueueJobBase {
    const DenseDesc *d;
    int idx;
    __device__ __forceinline__ explicit DenseJobBase(const DenseDesc *desc) : d(desc), idx(0) {}
    __device__ __forceinline__ QueueItem item(int i) {
        idx = i;
        int w = d->n + 1, h = 1 + d->m_ub + 2 * d->m_eq;
        if constexpr (F::free) w += d->n_free;
        if constexpr (F::bounds) h += d->n_upper;
        if constexpr (F::milp) h += d->n_bin;
        const int heven = (h + 1) & ~1;
        return QueueItem{w, h, (long long)((size_t)i * heven), (long long)((size_t)i * ((size_t)w + h)), d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int i, const QueueItem &it) const { return (long long)((size_t)i * it.w * it.h); }

    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        if constexpr (OUTLINE) dense_fill_call<T, F>(d, idx, it.w, it.h, mat, rhs, pos, var, lp);
        else dense_fill<T, F>(d, idx, it.w, it.h, mat, rhs, pos, var, lp);
    }
};

// ------------------------------------------------------------------------------------------
// The read-out: solution() (src/YALPS.ts:8-50) of one final tableau -- column 0, both permutations, width w, height h -- into
// x[0 .. n), the lanes striding along the variables; the return value is the objective (the caller's lane 0 writes it).
//   optimal    x[j] = v(1 + j) - v(twin[j]), v(column) solution()'s rule: col0 of the column's row where it is basic, above
//              precision rounded to it, anything else +0.0; the subtraction at a free variable alone; objective = -sign * result
//   unbounded  +0.0, +inf at the unbounded column `var[result]`, so -inf where that column is a twin; objective = sign * inf
//   neither    NaN
// then, where the call has lb and whatever the status, x[j] + l_eff[j], one addition per element (NaN + l_eff is NaN), and
// objective + shift_sum(c, l_eff), one addition after the rounding: wave 0 alone recomputes the sum, whole (the condition is the
// same for all lanes of a wave), from the caller's c, not sign * c.  The lane that owns j reads twin[j] and, for a free
// variable, one more pos entry: no barrier, no LDS.  Plain stores.
// SLICE = false, the LP jobs: col0 / pos / var are the queue's own of this LP, a basic row is `row >= 0`.
// SLICE = true, the MILP epilogue: they are a slice of the root's or the tree's buffers, whose height is the best node's: a basic
// row is tested against h, unsigned; x = nullptr: not wanted.
// ------------------------------------------------------------------------------------------
template <int T, class F, bool SLICE>
__device__ __forceinline__ double dense_readout(double *x, int n, const double *col0, const int32_t *pos, const int32_t *var, int w, int h,
                                                bool optimal, bool unbounded, const double *result, double sign, double p, const DenseLow &low,
                                                const double *c, long long cs) {
    const int tid = threadIdx.x, nx = SLICE && !x ? 0 : n;
    const double nan = __longlong_as_double(0x7ff8000000000000ll);
    auto shifted = [&](double xv, int j) { // x' + l_eff
        if constexpr (F::bounds) return low.l ? xv + low.at<F>(j) : xv;
        else return xv;
    };
    auto value = [&](int column) {
        const int row = pos[column] - w;
        const double v = (SLICE ? (unsigned)row < (unsigned)h : row >= 0) ? col0[row] : 0.0;
        return v > p ? round_to_precision(v, p) : 0.0;
    };
    double objective = nan;
    if (optimal) {
        for (int j = tid; j < nx; j += T) {
            int tj = -1;
            if constexpr (F::free) tj = low.twin[j];
            double xv = value(j + 1);
            if (tj >= 0) xv = xv - value(tj);
            x[j] = shifted(xv, j);
        }
        objective = -sign * *result;
    } else if (unbounded) {
        const int at = (int)*result;
        const int v = (unsigned)at < (unsigned)(w + h) ? var[at] : -1; // the unbounded column, 1-based
        for (int j = tid; j < nx; j += T) {
            int tj = -1;
            if constexpr (F::free) tj = low.twin[j];
            double xv = j + 1 == v ? INFINITY : 0.0;
            if (tj >= 0) xv = xv - (tj == v ? INFINITY : 0.0);
            x[j] = shifted(xv, j);
        }
        objective = sign * INFINITY;
    } else {
        for (int j = tid; j < nx; j += T) x[j] = nan;
    }
    if constexpr (F::bounds) {
        if (low.l && tid < 64) objective = objective + dense_shift_sum<F>(c, cs, low, n);
    }
    return objective;
}
