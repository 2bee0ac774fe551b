// lp_sens_kernel.cuh -- lp_batch_kernel plus a ranging epilogue over the final tableau of every LP that ended optimal
// Part of libyalps_lpsens.so; included by lp_sens.hip inside its anonymous namespace (gfx950 only).
#pragma once

// ------------------------------------------------------------------------------------------
// lp_sens_kernel: lp_batch_kernel's body (lp_batch_kernel.cuh: the work queue, the barriers, the assembly from cells,
// wg_simplex unchanged), and between wg_simplex and the last barrier of an LP that ended "optimal" two passes over the
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
struct LpDesc {
    int32_t w, h;
    long long cell_lo, cell_hi;   // the LP's cells in the packed row / col / val arrays
    long long col0_off;           // column 0 at col0[col0_off .. + h)
    long long perm_off;           // the permutations at pos / var[perm_off .. + w + h); the ranges at sens[3 * perm_off ..)
    long long tab_off;            // keep_tableaux: the final matrix, row-major w * h, at tab[tab_off ..)
    double precision, max_pivots;
    int32_t aux_hbm;              // HBM form: colbuf / prow behind the tableau in the workspace (too long for the LDS block)
    int32_t pad_;
};

struct LpLaunch {
    const LpDesc *desc;           // [LPs of the batch]
    const int32_t *order;         // [count] LP indices of this launch, largest first
    int32_t count;
    unsigned int *counter;        // next entry of `order` to hand out (zeroed before the launch)
    const int32_t *row, *col;
    const double *val;
    int32_t *status;              // per LP of the batch
    double *result;
    long long *pivots;
    double *col0;
    int32_t *pos, *var;
    double *tab;                  // nullptr unless keep_tableaux
    double *ws;                   // HBM form: [grid][ws_stride]
    long long ws_stride;
    int32_t *hist;                // checkCycles: [grid][2][hist_cap] pivot history of the LP a workgroup is solving
    long long hist_cap;
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

// The dynamic LDS block holds the tableau and prow, which wg_simplex sweeps 16 bytes at a time: it must start on a 16-byte
// boundary, so the static objects in front of it add up to a multiple of 16 (the queue slot is padded to 16 bytes;
// build.build_lpsens refuses a library whose kernels' static LDS is not).
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_sens_kernel(LpLaunch L) {
    __shared__ double sk[2][16];
    __shared__ int si[2][16];
    __shared__ __attribute__((aligned(16))) unsigned int s_next[4]; // [0]: the queue index this workgroup works on next
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    const int tid = threadIdx.x;
    if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u);
    __syncthreads();
    // The loop's top only READS the index; the one lane that fetches the next one does so in the middle of the body, between
    // two barriers, and the body ends with a barrier.  No per-lane block touches the back edge, so the loop stays uniform
    // however the compiler threads branches (lp_batch_kernel.cuh tells what happened when one did).  The epilogue keeps to
    // that: it sits between the outputs and the last barrier, under a condition every lane shares.
    for (;;) {
        const unsigned int k = __builtin_amdgcn_readfirstlane(s_next[0]);
        if (k >= (unsigned int)L.count) return;
        const int i = L.order[k];
        const LpDesc *d = L.desc + i;
        const int w = d->w, h = d->h, n = w - 1;
        const int pcols = small_pcols(n), lp = LDS ? small_lds_pitch(n) : pcols;
        const long long cell_lo = d->cell_lo, cell_hi = d->cell_hi, col0_off = d->col0_off, perm_off = d->perm_off;
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
            prow = d->aux_hbm ? mat + (size_t)h * lp : sh_dyn;
            colbuf = prow + lp;
        }
        // ---- the initial tableau (src/tableau.ts:87-134): zeros, the written cells, identity permutations ----
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
        __syncthreads();
        if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u); // (everybody read the slot two barriers ago; read again after the last one)

        int32_t *hist_l = CHECK ? L.hist + (size_t)blockIdx.x * 2 * L.hist_cap : nullptr;
        const WgResult out = wg_simplex<T, CHECK>(mat, rhs, pos, var, colbuf, prow, sk, si, w, n, lp, pcols, h,
                                                  wg_unit_lanes(pcols / 2, T), d->precision, d->max_pivots, hist_l,
                                                  CHECK ? hist_l + L.hist_cap : nullptr, CHECK ? L.hist_cap : 0);
        __syncthreads();
        // (checkCycles, history full: no output but the status -- the host grows the history and reruns this LP)
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
            double *tab = L.tab + d->tab_off;
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
        // (last: by now only the tableau itself is still needed, which keeps the epilogue's registers off the solve's)
        if (out.status == YALPS_OPTIMAL) sens_epilogue<T>(mat, rhs, w, h, lp, d->precision, L.sens + 3 * perm_off);
        __syncthreads(); // everybody is done with this LP's tableau, and the next index is in its slot
    }
}
