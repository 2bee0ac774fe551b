// lp_batch_kernel.cuh -- a batch of independent LPs of different shapes, one workgroup per LP at a time
// Part of libyalps_lpbatch.so; included by lp_batch.hip inside its anonymous namespace (gfx950 only).
#pragma once

// ------------------------------------------------------------------------------------------
// lp_batch_kernel: every LP of a launch is solved from start to finish by ONE workgroup -- tableauModel's cells in,
// what solution() reads out -- and a launch covers LPs of any mix of shapes.  Workgroups do not own an LP: each takes
// the next index of the launch's order (largest LP first) from a device counter until the counter passes the count, so
// LPs whose pivot counts differ by orders of magnitude still fill the chip.  There is no waiting between workgroups of
// any kind: a workgroup that is not resident yet simply takes its first index later.
// Per LP: zero the tableau, scatter the cells (column 0 into rhs, the rest at mat[r * lp + c - 1]), identity
// permutations (src/tableau.ts:95-98), then wg_simplex (wg_simplex.cuh) unchanged.
// LDS = true: tableau, rhs, colbuf, prow and both permutations in LDS, small_kernel's layout (small_lds_pitch).
// LDS = false: the tableau in this workgroup's workspace in HBM (L2-resident while it is worked on), column 0 and the
// permutations directly at the LP's output offsets, colbuf / prow in LDS where they fit the launch's allocation.
// ------------------------------------------------------------------------------------------
struct LpDesc {
    int32_t w, h;
    long long cell_lo, cell_hi;   // the LP's cells in the packed row / col / val arrays
    long long col0_off;           // column 0 at col0[col0_off .. + h)
    long long perm_off;           // the permutations at pos / var[perm_off .. + w + h)
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
};

// The dynamic LDS block holds the tableau and prow, which wg_simplex sweeps 16 bytes at a time: it must start on a 16-byte
// boundary, so the static objects in front of it add up to a multiple of 16 (the queue slot is padded to 16 bytes;
// build.build_lpbatch refuses a library whose kernels' static LDS is not).
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void lp_batch_kernel(LpLaunch L) {
    __shared__ double sk[2][16];
    __shared__ int si[2][16];
    __shared__ __attribute__((aligned(16))) unsigned int s_next[4]; // [0]: the queue index this workgroup works on next
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    const int tid = threadIdx.x;
    if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u);
    __syncthreads();
    // The loop's top only READS the index; the one lane that fetches the next one does so in the middle of the body, between
    // two barriers, and the body ends with a barrier.  No per-lane block touches the back edge, so the loop stays uniform
    // however the compiler threads branches (a `tid == 0` fetch at the top next to a one-lane record at the bottom was merged
    // across the back edge by hipcc: lane 0 left the body on a path of its own, its wave-mates met the next s_barrier without
    // it and the kernel never ended).
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
        __syncthreads(); // everybody is done with this LP's tableau, and the next index is in its slot
    }
}
