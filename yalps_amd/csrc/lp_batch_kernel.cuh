// lp_batch_kernel.cuh -- a batch of independent LPs of different shapes, one workgroup per LP at a time
// Part of libyalps_lpbatch.so; included by lp_batch.hip inside its anonymous namespace (gfx950 only).
#pragma once
#include "wg_queue.cuh"

// ------------------------------------------------------------------------------------------
// lp_batch_kernel: every LP of a launch is solved from start to finish by ONE workgroup -- tableauModel's cells in,
// what solution() reads out -- and a launch covers LPs of any mix of shapes, handed out by wg_queue (wg_queue.cuh).
// Per LP: zero the tableau, scatter the cells (column 0 into rhs, the rest at mat[r * lp + c - 1]), identity
// permutations (src/tableau.ts:95-98), then wg_simplex (wg_simplex.cuh) unchanged.
// ------------------------------------------------------------------------------------------
struct LpDesc {
    int32_t w, h;
    long long cell_lo, cell_hi;   // the LP's cells in the packed row / col / val arrays
    long long col0_off;           // column 0 at col0[col0_off .. + h)
    long long perm_off;           // the permutations at pos / var[perm_off .. + w + h); lp_sens_kernel: the ranges at sens[3 * perm_off ..)
    long long tab_off;            // keep_tableaux: the final matrix, row-major w * h, at tab[tab_off ..)
    double precision, max_pivots;
    int32_t aux_hbm;              // HBM form: colbuf / prow behind the tableau in the workspace (too long for the LDS block)
    int32_t pad_;
};

struct LpLaunch : QueueLaunch {
    const LpDesc *desc;           // [LPs of the batch]
    const int32_t *row, *col;
    const double *val;
};

// the initial tableau (src/tableau.ts:87-134): zeros, the written cells, identity permutations
struct LpJob : QueueJobBase {
    const LpLaunch &L;
    const LpDesc *d;
    long long cell_lo, cell_hi;
    __device__ __forceinline__ explicit LpJob(const LpLaunch &launch) : L(launch) {}
    __device__ __forceinline__ QueueItem item(int i) {
        d = L.desc + i;
        cell_lo = d->cell_lo;
        cell_hi = d->cell_hi;
        return QueueItem{d->w, d->h, d->col0_off, d->perm_off, d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int, const QueueItem &) const { return d->tab_off; }
    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        const int tid = threadIdx.x, w = it.w, h = it.h;
        {
            double2 *m2 = reinterpret_cast<double2 *>(mat);
            const size_t units = (size_t)h * lp / 2; // lp is even
            for (size_t u = tid; u < units; u += T) m2[u] = make_double2(0.0, 0.0);
            for (int r = tid; r < h; r += T) rhs[r] = 0.0;
            for (int p = tid; p < w + h; p += T) {
                pos[p] = p;
                var[p] = p;
            }
        }
        __syncthreads();
        for (long long c = cell_lo + tid; c < cell_hi; c += T) {
            const int r = L.row[c], cc = L.col[c];
            if ((unsigned)r >= (unsigned)h || (unsigned)cc >= (unsigned)w) continue; // (the host has refused such cells)
            if (cc == 0)
                rhs[r] = L.val[c];
            else
                mat[(size_t)r * lp + cc - 1] = L.val[c];
        }
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_batch_kernel(LpLaunch L) {
    wg_queue<T, CHECK, LDS>(L, LpJob(L));
}
