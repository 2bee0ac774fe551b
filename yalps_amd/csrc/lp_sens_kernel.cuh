// lp_sens_kernel.cuh -- lp_batch_kernel plus a ranging epilogue over the final tableau of every LP that ended optimal
// Part of libyalps_lpsens.so; included by lp_sens.hip inside its anonymous namespace (gfx950 only).
#pragma once
#include "lp_batch_kernel.cuh"

// ------------------------------------------------------------------------------------------
// lp_sens_kernel: lp_batch_kernel's job on wg_queue (lp_batch_kernel.cuh: the assembly from cells; wg_queue.cuh: the work
// queue, the barriers, wg_simplex unchanged), and between wg_simplex and the last barrier of an LP that ended "optimal" two passes over the
// final matrix M where it lies (LDS in the LDS form, the workgroup's HBM workspace in the HBM form), p = the LP's precision:
//   row0[c]   = M[0,c]                                                        c = 0 .. w-1
//   col_up[c] = min{ M[r,0] /  M[r,c] : 1 <= r < h, M[r,c] >  p }             c = 1 .. w-1   (+inf where empty)
//   col_dn[c] = min{ M[r,0] / -M[r,c] : 1 <= r < h, M[r,c] < -p }                            (+inf where empty)
//   row_lo[r] = max{ M[0,c] /  M[r,c] : 1 <= c < w, M[r,c] >  p }             r = 1 .. h-1   (-inf where empty)
//   row_hi[r] = min{ M[0,c] /  M[r,c] : 1 <= c < w, M[r,c] < -p }                            (+inf where empty)
// Entry 0 of the four ratio arrays is 0.0; every quotient is one IEEE division; a NaN quotient is ignored (fmin / fmax).
// Layout of the epilogue: a group of G lanes (a power of two, at most a wave) owns a column (first pass) or a row (second
// pass); its lanes stride over the rows (columns), keep a running fmin / fmax, and fold it with log2(G) lane exchanges
// inside the wave.  No LDS beyond lp_batch_kernel's, no barrier: the epilogue only reads the tableau, and every lane writes
// straight to the LP's slice of the output.  Columns 1 .. w-1 only: the padding column of an odd n is never read.
// The LP's slice: sens[3 * perm_off ..) = row0[w] col_up[w] col_dn[w] row_lo[h] row_hi[h].
// ------------------------------------------------------------------------------------------
struct SensLaunch : LpLaunch {
    double *sens;                 // the ranges of every LP that ends optimal
};

// lanes of a wave that share a line of `count` entries: the power of two >= count, at most 64
__device__ inline int sens_group_lanes(int count) {
    int g = 1;
    while (g < count && g < 64) g *= 2;
    return g;
}

// The ranging epilogue.  Every lane of the workgroup calls it (the lane exchanges need whole groups); it has no barrier.
// A function of its own, not inlined: inlined, its registers came on top of wg_simplex's in the allocator's eyes and the
// <1024,check> HBM instantiation, five registers under the 128 a workgroup of 1024 lanes may use, spilled to scratch.
template <int T>
__device__ __attribute__((noinline)) void sens_epilogue(const double *mat, const double *rhs, int w, int h, int lp,
                                                             double p, double *out) {
    const int tid = threadIdx.x;
    double *row0 = out, *col_up = out + w, *col_dn = col_up + w, *row_lo = col_dn + w, *row_hi = row_lo + h;
    for (int c = tid; c < w; c += T) row0[c] = c == 0 ? rhs[0] : mat[c - 1];
    if (tid == 0) {
        col_up[0] = 0.0;
        col_dn[0] = 0.0;
        row_lo[0] = 0.0;
        row_hi[0] = 0.0;
    }
    { // columns: G lanes walk the rows of one column
        const int G = sens_group_lanes(h - 1), l = tid % G, NG = T / G;
        for (int c0 = 1; c0 < w; c0 += NG) { // (uniform trip count: every lane of a group takes part in the exchange)
            const int c = c0 + tid / G;
            double up = INFINITY, dn = INFINITY;
            if (c < w)
#pragma unroll 1
                for (int r = 1 + l; r < h; r += G) {
                    const double v = mat[(size_t)r * lp + c - 1], b = rhs[r];
                    const bool above = v > p, below = v < -p;
                    if (!(above || below)) continue;
                    const double q = b / v; // (b / -v is -(b / v) bit for bit: one division serves both sides)
                    if (above) up = fmin(up, q);
                    if (below) dn = fmin(dn, -q);
                }
            for (int s = G >> 1; s > 0; s >>= 1) {
                up = fmin(up, __shfl_xor(up, s));
                dn = fmin(dn, __shfl_xor(dn, s));
            }
            if (l == 0 && c < w) {
                col_up[c] = up;
                col_dn[c] = dn;
            }
        }
    }
    { // rows: G lanes walk the columns of one row
        const int G = sens_group_lanes(w - 1), l = tid % G, NG = T / G;
        for (int r0 = 1; r0 < h; r0 += NG) {
            const int r = r0 + tid / G;
            double lo = -INFINITY, hi = INFINITY;
            if (r < h) {
                const double *mrow = mat + (size_t)r * lp;
#pragma unroll 1
                for (int c = 1 + l; c < w; c += G) {
                    const double v = mrow[c - 1], k = mat[c - 1];
                    const bool above = v > p, below = v < -p;
                    if (!(above || below)) continue;
                    const double q = k / v;
                    if (above) lo = fmax(lo, q);
                    if (below) hi = fmin(hi, q);
                }
            }
            for (int s = G >> 1; s > 0; s >>= 1) {
                lo = fmax(lo, __shfl_xor(lo, s));
                hi = fmin(hi, __shfl_xor(hi, s));
            }
            if (l == 0 && r < h) {
                row_lo[r] = lo;
                row_hi[r] = hi;
            }
        }
    }
}

// lp_batch_kernel's job with the epilogue between the outputs and the last barrier, under a condition every lane shares
struct SensJob : LpJob {
    const SensLaunch &S;
    __device__ __forceinline__ explicit SensJob(const SensLaunch &launch) : LpJob(launch), S(launch) {}
    template <int T>
    __device__ __forceinline__ void after(const QueueItem &it, int status, const double *mat, const double *rhs, int lp) const {
        if (status == YALPS_OPTIMAL) sens_epilogue<T>(mat, rhs, it.w, it.h, lp, d->precision, S.sens + 3 * it.perm_off);
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_sens_kernel(SensLaunch L) {
    wg_queue<T, CHECK, LDS>(L, SensJob(L));
}
