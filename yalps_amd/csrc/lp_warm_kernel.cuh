// lp_warm_kernel.cuh -- many variants of ONE LP, each restarted from the base's OPTIMAL tableau: one workgroup per variant at a time
// Part of libyalps_lpwarm.so; included by lp_warm.hip inside its anonymous namespace (gfx950 only).
#pragma once
#include "wg_queue.cuh"

// ------------------------------------------------------------------------------------------
// A variant that moves only right-hand sides (column 0 of the initial tableau) and objective coefficients (row 0) leaves
// the body of the base's final tableau F valid: in the basis F stands in, the variant's tableau differs from F in column 0
// and row 0 alone.  The host solves the base once (lp_batch_kernel, tableau kept), lp_warm_image_kernel repacks the kept
// matrix into the image layout of lp_variants_kernel.cuh (the matrix at the form's row pitch, column 0 behind it, even
// length), and the host turns every patch cell into a *record* (p, d): d = the cell's new value minus its value in the
// base's initial tableau, p = where the base's final permutation put the cell's slack (column 0 cells) or variable (row 0
// cells).  lp_warm_kernel starts every variant from a copy of the image and the base's permutations, folds the records in
//   column 0, in patch order:   p < w:  M[i,0] = M[i,0] + d * M[i,p]   for every row i (row 0 included)
//                               else:   M[p-w,0] += d
//   row 0, in patch order:      p < w:  M[0,p] += d
//                               else:   M[0,j] = M[0,j] - d * M[p-w,j]  for every column j (column 0, as the column 0 records left it, included)
// every product and every sum rounded on its own, and from there on it is lp_batch_kernel: the same work queue (wg_queue.cuh),
// wg_simplex unchanged -- its phase 1 repairs a right-hand side that went negative from any basis -- and the same outputs.
// ------------------------------------------------------------------------------------------

// the kept final matrix of the base (row-major w * h, column 0 included) into the image of this call's form
__global__ __launch_bounds__(256) void lp_warm_image_kernel(double *image, long long image_doubles, const double *tab, int w, int h,
                                                            int pitch) {
    const long long stride = (long long)gridDim.x * blockDim.x, body = (long long)h * pitch;
    for (long long u = (long long)blockIdx.x * blockDim.x + threadIdx.x; u < image_doubles; u += stride) {
        double v = 0.0; // (the pitch's padding columns and the closing pad of an odd h)
        if (u < body) {
            const long long r = u / pitch;
            const int c = (int)(u - r * pitch);
            if (c < w - 1) v = tab[(size_t)r * w + c + 1];
        } else if (u - body < h) {
            v = tab[(size_t)(u - body) * w];
        }
        image[u] = v;
    }
}

struct WarmDesc {
    long long c0_lo, r0_lo, r0_hi; // the variant's records in rec_p / rec_d: column 0 at [c0_lo, r0_lo), row 0 at [r0_lo, r0_hi)
    double precision, max_pivots;
};

struct WarmLaunch : QueueLaunch {
    const WarmDesc *desc;         // [variants of the call]; outputs laid out as lp_variants_kernel's
    int32_t w, h;
    int32_t aux_hbm;              // HBM form: colbuf / prow behind the tableau in the workspace (too long for the LDS block)
    const double *image;          // [h * pitch + even(h)] the base's final tableau in this form's layout
    const int32_t *bpos, *bvar;   // [w + h] the base's final permutations
    const int32_t *rec_p;         // the records
    const double *rec_d;
};

// Column 0 and row 0 of the variant in the base's final basis.  Every lane calls it; the barrier between the two steps is
// its own.  A function of its own, not inlined, as lp_sens_kernel's epilogue and for its reason: inlined, its registers
// come on top of wg_simplex's in the allocator's eyes, and <1024,check> in the HBM form is five registers under its limit.
// Step 1: a lane owns rows tid, tid + T, ...; it keeps the row's column 0 value in a register and folds every record into
// it in order -- a row depends on nothing but itself, so no barrier between records.  In LDS the lanes of a wave read one
// column of consecutive rows: the pitch (2 * odd doubles) spreads them over 16 of the 32 eight-byte bank pairs, a 2-way
// conflict at worst, as in wg_simplex's own column reads.  Step 2: a lane owns columns (column 0 among them) and reads a row
// at consecutive addresses.  The record lists are read at indices every lane shares.
template <int T>
__device__ __attribute__((noinline)) void warm_update(double *mat, double *rhs, int w, int h, int lp, const int32_t *rec_p,
                                                      const double *rec_d, long long c0_lo, long long r0_lo, long long r0_hi) {
    const int tid = threadIdx.x;
    if (c0_lo < r0_lo)
        for (int i = tid; i < h; i += T) {
            const double *mrow = mat + (size_t)i * lp;
            double v = rhs[i];
#pragma unroll 1
            for (long long k = c0_lo; k < r0_lo; k++) {
                const int p = rec_p[k];
                const double d = rec_d[k];
                if (p < w) {
                    if (p >= 1) { // (the host sends no other: a slack is never at position 0)
                        const double t = d * mrow[p - 1];
                        v = v + t;
                    }
                } else if (p - w == i) {
                    v = v + d;
                }
            }
            rhs[i] = v;
        }
    __syncthreads();
    if (r0_lo < r0_hi)
        for (int j = tid; j < w; j += T) {
            double *cell = j == 0 ? rhs : mat + (j - 1);
            double v = *cell;
#pragma unroll 1
            for (long long k = r0_lo; k < r0_hi; k++) {
                const int p = rec_p[k];
                const double d = rec_d[k];
                if (p < w) {
                    if (p == j) v = v + d;
                } else if (p - w >= 1 && p - w < h) { // (the host sends no other: row 0 holds no variable)
                    const int r = p - w;
                    const double t = d * (j == 0 ? rhs[r] : mat[(size_t)r * lp + j - 1]);
                    v = v - t;
                }
            }
            *cell = v;
        }
}

// the initial tableau: the image, the base's permutations, then the records
struct WarmJob : QueueJobBase {
    const WarmLaunch &L;
    const WarmDesc *d;
    long long c0_lo, r0_lo, r0_hi;
    __device__ __forceinline__ explicit WarmJob(const WarmLaunch &launch) : L(launch) {}
    __device__ __forceinline__ QueueItem item(int i) {
        d = L.desc + i;
        c0_lo = d->c0_lo;
        r0_lo = d->r0_lo;
        r0_hi = d->r0_hi;
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
                pos[p] = L.bpos[p];
                var[p] = L.bvar[p];
            }
        }
        __syncthreads();
        if (c0_lo < r0_hi) warm_update<T>(mat, rhs, w, h, lp, L.rec_p, L.rec_d, c0_lo, r0_lo, r0_hi); // (the same in every lane)
    }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_warm_kernel(WarmLaunch L) {
    wg_queue<T, CHECK, LDS>(L, WarmJob(L));
}
