// lp_variants_kernel.cuh -- many variants of ONE LP: a shared base tableau plus a small patch per variant, one workgroup per variant at a time
// Part of libyalps_lpvar.so; included by lp_variants.hip inside its anonymous namespace (gfx950 only).
#pragma once
#include "wg_queue.cuh"

// ------------------------------------------------------------------------------------------
// All variants of a call have one shape, so the call has one size class and one *image*: the base tableau, dense, in the
// layout the solving kernel starts from -- the matrix at the form's row pitch (small_lds_pitch(n) for the LDS form,
// small_pcols(n) for the HBM form; element (r, c >= 1) at image[r * pitch + c - 1]) followed by column 0 (h doubles, then
// one zero where h is odd, so that the image is a whole number of 16-byte units).
// lp_variants_base_kernel builds the image once per call; lp_variants_kernel starts every variant from it: a 16-byte copy
// per lane per step instead of lp_batch_kernel's zero pass plus the scatter of the whole cell list, then the variant's few
// patch cells on top.  From there on it is lp_batch_kernel: the same work queue (wg_queue.cuh), wg_simplex unchanged, the same outputs.
// ------------------------------------------------------------------------------------------

// scatter == 0: zero the image; scatter != 0: write the base cells into it.  Two launches of one kernel, ordered by the
// stream (a cell may not be overtaken by the zero of its own word); the solving launches follow on the same stream.
__global__ __launch_bounds__(256) void lp_variants_base_kernel(double *image, long long image_doubles, const int32_t *row,
                                                               const int32_t *col, const double *val, long long ncells, int w,
                                                               int h, int pitch, int scatter) {
    const long long stride = (long long)gridDim.x * blockDim.x, first = (long long)blockIdx.x * blockDim.x + threadIdx.x;
    if (!scatter) {
        double2 *im2 = reinterpret_cast<double2 *>(image);
        for (long long u = first; u < image_doubles / 2; u += stride) im2[u] = make_double2(0.0, 0.0); // image_doubles is even
        return;
    }
    for (long long c = first; c < ncells; c += stride) {
        const int r = row[c], cc = col[c];
        if ((unsigned)r >= (unsigned)h || (unsigned)cc >= (unsigned)w) continue; // (the host has refused such cells)
        if (cc == 0)
            image[(size_t)h * pitch + r] = val[c];
        else
            image[(size_t)r * pitch + cc - 1] = val[c];
    }
}

struct VarDesc {
    long long patch_lo, patch_hi; // the variant's patch in the packed patch_row / patch_col / patch_val arrays
    double precision, max_pivots;
};

struct VarLaunch : QueueLaunch {
    const VarDesc *desc;          // [variants of the call]; variant i has column 0 at col0[i * even(h)], the permutations
    int32_t w, h;                 // at pos / var[i * (w + h)], with keep_tableaux the final matrix at tab[i * w * h]
    int32_t aux_hbm;              // HBM form: colbuf / prow behind the tableau in the workspace (too long for the LDS block)
    const double *image;          // [h * pitch + even(h)] the base tableau in this form's layout
    const int32_t *prow, *pcol;   // the patches
    const double *pval;
};

// the initial tableau: the base image, identity permutations (src/tableau.ts:95-98), then the patch
struct VarJob : QueueJobBase {
    const VarLaunch &L;
    const VarDesc *d;
    long long patch_lo, patch_hi;
    __device__ __forceinline__ explicit VarJob(const VarLaunch &launch) : L(launch) {}
    __device__ __forceinline__ QueueItem item(int i) {
        d = L.desc + i;
        patch_lo = d->patch_lo;
        patch_hi = d->patch_hi;
        const int w = L.w, h = L.h, heven = (h + 1) & ~1;
        return QueueItem{w, h, (long long)((size_t)i * heven), (long long)((size_t)i * ((size_t)w + h)), L.aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return d->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int i, const QueueItem &it) const { return (long long)((size_t)i * it.w * it.h); }
    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        const int tid = threadIdx.x, w = it.w, h = it.h, heven = (h + 1) & ~1;
        {
            const double2 *im2 = reinterpret_cast<const double2 *>(L.image);
            double2 *m2 = reinterpret_cast<double2 *>(mat);
            const size_t munits = (size_t)h * lp / 2; // lp is even
            if (LDS) {
                // rhs follows the matrix in LDS as column 0 follows it in the image: one run (h odd: the image's closing zero
                // lands in colbuf[0], which every pivot writes before it reads)
                const size_t units = munits + heven / 2;
                for (size_t u = tid; u < units; u += T) m2[u] = im2[u];
            } else {
                for (size_t u = tid; u < munits; u += T) m2[u] = im2[u];
                double2 *r2 = reinterpret_cast<double2 *>(rhs); // (column 0 slots are even(h) doubles apart: 16-byte aligned, the pad is this variant's own)
                for (int u = tid; u < heven / 2; u += T) r2[u] = im2[munits + u];
            }
            for (int p = tid; p < w + h; p += T) {
                pos[p] = p;
                var[p] = p;
            }
        }
        __syncthreads();
        for (long long c = patch_lo + tid; c < patch_hi; c += T) {
            const int r = L.prow[c], cc = L.pcol[c];
            if ((unsigned)r >= (unsigned)h || (unsigned)cc >= (unsigned)w) continue; // (the host has refused such cells)
            if (cc == 0)
                rhs[r] = L.pval[c];
            else
                mat[(size_t)r * lp + cc - 1] = L.pval[c];
        }
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_variants_kernel(VarLaunch L) {
    wg_queue<T, CHECK, LDS>(L, VarJob(L));
}
