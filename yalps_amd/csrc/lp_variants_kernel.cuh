// lp_variants_kernel.cuh -- many variants of ONE LP: a shared base tableau plus a small patch per variant, one workgroup per variant at a time
// Part of libyalps_lpvar.so; included by lp_variants.hip inside its anonymous namespace (gfx950 only).
#pragma once

// ------------------------------------------------------------------------------------------
// All variants of a call have one shape, so the call has one size class and one *image*: the base tableau, dense, in the
// layout the solving kernel starts from -- the matrix at the form's row pitch (small_lds_pitch(n) for the LDS form,
// small_pcols(n) for the HBM form; element (r, c >= 1) at image[r * pitch + c - 1]) followed by column 0 (h doubles, then
// one zero where h is odd, so that the image is a whole number of 16-byte units).
// lp_variants_base_kernel builds the image once per call; lp_variants_kernel starts every variant from it: a 16-byte copy
// per lane per step instead of lp_batch_kernel's zero pass plus the scatter of the whole cell list, then the variant's few
// patch cells on top.  From there on it is lp_batch_kernel: the same work queue, wg_simplex unchanged, the same outputs.
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

struct VarLaunch {
    const VarDesc *desc;          // [variants of the call]
    const int32_t *order;         // [count] variant indices of this launch
    int32_t count;
    unsigned int *counter;        // next entry of `order` to hand out (zeroed before the launch)
    int32_t w, h;                 // the one shape of the call
    int32_t aux_hbm;              // HBM form: colbuf / prow behind the tableau in the workspace (too long for the LDS block)
    const double *image;          // [h * pitch + even(h)] the base tableau in this form's layout
    const int32_t *prow, *pcol;   // the patches
    const double *pval;
    int32_t *status;              // per variant; variant i has column 0 at col0[i * even(h)], the permutations at
    double *result;               // pos / var[i * (w + h)], with keep_tableaux the final matrix at tab[i * w * h]
    long long *pivots;
    double *col0;
    int32_t *pos, *var;
    double *tab;                  // nullptr unless keep_tableaux
    double *ws;                   // HBM form: [grid][ws_stride]
    long long ws_stride;
    int32_t *hist;                // checkCycles: [grid][2][hist_cap] pivot history of the variant a workgroup is solving
    long long hist_cap;
};

// Static LDS in front of the dynamic block adds up to a multiple of 16 bytes, as in lp_batch_kernel (the dynamic block holds
// the tableau and prow, swept 16 bytes at a time; build.build_lpvar refuses a library whose kernels' static LDS is not).
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_variants_kernel(VarLaunch L) {
    __shared__ double sk[2][16];
    __shared__ int si[2][16];
    __shared__ __attribute__((aligned(16))) unsigned int s_next[4]; // [0]: the queue index this workgroup works on next
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    const int tid = threadIdx.x;
    const int w = L.w, h = L.h, n = w - 1;
    const int pcols = small_pcols(n), lp = LDS ? small_lds_pitch(n) : pcols;
    const int heven = (h + 1) & ~1;
    if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u);
    __syncthreads();
    // The loop's shape is lp_batch_kernel's (see the comment there): the top only READS the index, one lane fetches the next
    // one in the middle of the body between two barriers, and the body ends with a barrier -- nothing per-lane at the back edge.
    for (;;) {
        const unsigned int k = __builtin_amdgcn_readfirstlane(s_next[0]);
        if (k >= (unsigned int)L.count) return;
        const int i = L.order[k];
        const VarDesc *d = L.desc + i;
        const long long patch_lo = d->patch_lo, patch_hi = d->patch_hi;
        const size_t col0_off = (size_t)i * heven, perm_off = (size_t)i * ((size_t)w + h);
        double *mat, *rhs, *colbuf, *prow;
        int32_t *pos, *var;
        if (LDS) {
            mat = sh_dyn;
            rhs = mat + (size_t)h * lp;
            colbuf = rhs + h;
            prow = colbuf + h;
            pos = reinterpret_cast<int32_t *>(prow + lp);
            var = pos + ((w + h + 1) & ~1);
        } else {
            mat = L.ws + (size_t)blockIdx.x * L.ws_stride;
            rhs = L.col0 + col0_off;
            pos = L.pos + perm_off;
            var = L.var + perm_off;
            prow = L.aux_hbm ? mat + (size_t)h * lp : sh_dyn;
            colbuf = prow + lp;
        }
        // ---- the initial tableau: the base image, identity permutations (src/tableau.ts:95-98), then the patch ----
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
        __syncthreads();
        if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u); // (everybody read the slot two barriers ago; read again after the last one)

        int32_t *hist_l = CHECK ? L.hist + (size_t)blockIdx.x * 2 * L.hist_cap : nullptr;
        const WgResult out = wg_simplex<T, CHECK>(mat, rhs, pos, var, colbuf, prow, sk, si, w, n, lp, pcols, h,
                                                  wg_unit_lanes(pcols / 2, T), d->precision, d->max_pivots, hist_l,
                                                  CHECK ? hist_l + L.hist_cap : nullptr, CHECK ? L.hist_cap : 0);
        __syncthreads();
        // (checkCycles, history full: no output but the status -- the host grows the history and reruns this variant from the image)
        const bool done = !(CHECK && out.status == WG_HISTORY_FULL);
        if (LDS && done) {
            double *col0 = L.col0 + col0_off;
            for (int r = tid; r < h; r += T) col0[r] = rhs[r];
            int32_t *opos = L.pos + perm_off, *ovar = L.var + perm_off;
            for (int p = tid; p < w + h; p += T) {
                opos[p] = pos[p];
                ovar[p] = var[p];
            }
        }
        if (L.tab && done) { // the whole final matrix in the reference's layout (src/tableau.ts:9-21)
            double *tab = L.tab + (size_t)i * w * h;
            const int Uc = wg_unit_lanes(w, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
            for (int r = cg0; r < h; r += CG) {
                const double *src = mat + (size_t)r * lp;
                double *dst = tab + (size_t)r * w;
                for (int c = cu0; c < w; c += Uc) dst[c] = c == 0 ? rhs[r] : src[c - 1];
            }
        }
        if (tid == T - 1) {
            L.status[i] = out.status;
            if (done) {
                L.result[i] = out.result;
                L.pivots[i] = out.pivots;
            }
        }
        __syncthreads(); // everybody is done with this variant's tableau, and the next index is in its slot
    }
}
