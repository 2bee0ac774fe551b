// milp_node_kernel.cuh -- branch-and-cut nodes of many roots of different shapes, one workgroup per node at a time
// Part of libyalps_milpbatch.so; included by milp_batch.hip inside its anonymous namespace (gfx950 only).
#pragma once

// ------------------------------------------------------------------------------------------
// milp_node_kernel: lp_batch_kernel's work queue (one launch covers nodes of any mix of roots and shapes, handed out
// largest first from a device counter, no waiting between workgroups) around batch_kernel's applyCuts
// (src/branchAndCut.ts:22-61).  The roots are the optimal tableaux the root pass (lp_batch_kernel, kept tableaux) left on
// the device: row-major width x height with column 0 in front, permutations at the root's perm_off.  A node is its root
// plus one row per cut; it is solved by wg_simplex (wg_simplex.cuh) unchanged with the ROOT's precision and checkCycles and
// the node's pivot budget (the root's maxPivots, src/branchAndCut.ts:127, unless the host overrides it).
// LDS = true: the node's tableau, rhs, colbuf, prow and both permutations in LDS, small_kernel's layout (small_lds_pitch).
// LDS = false: the tableau in this workgroup's workspace in HBM, column 0 and the permutations directly at the node's
// output offsets, colbuf / prow in LDS where they fit the launch's allocation.
// ------------------------------------------------------------------------------------------
struct NodeDesc {
    int32_t root;                 // index into the roots of the last root pass
    int32_t ncuts;
    long long cut_lo;             // the node's cuts at cut_sign / cut_var / cut_val[cut_lo .. + ncuts)
    long long col0_off;           // column 0 at col0[col0_off .. + h)
    long long perm_off;           // the permutations at pos / var[perm_off .. + w + h)
    long long tab_off;            // keep_tableaux: the final matrix, row-major w * h, at tab[tab_off ..)
    double max_pivots;
    int32_t aux_hbm;              // HBM form: colbuf / prow behind the tableau in the workspace
    int32_t pad_;
};

struct NodeLaunch {
    const LpDesc *roots;          // [roots]: w, h, tab_off, perm_off, precision of every root
    const double *root_tab;       // the roots' final matrices
    const int32_t *root_pos, *root_var;
    const NodeDesc *node;         // [nodes of the pass]
    const int32_t *order;         // [count] node indices of this launch, largest first
    int32_t count;
    unsigned int *counter;        // next entry of `order` to hand out (zeroed before the launch)
    const int32_t *cut_sign, *cut_var;
    const double *cut_val;
    int32_t *status, *height;     // per node of the pass
    double *result;
    long long *pivots;
    double *col0;
    int32_t *pos, *var;
    double *tab;                  // nullptr unless keep_tableaux
    double *ws;                   // HBM form: [grid][ws_stride]
    long long ws_stride;
    int32_t *hist;                // checkCycles: [grid][2][hist_cap]
    long long hist_cap;
};

// Static LDS in front of the dynamic block adds up to a multiple of 16 bytes, as in lp_batch_kernel
// (build.check_register_budgets refuses a library where it does not).
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_node_kernel(NodeLaunch L) {
    __shared__ double sk[2][16];
    __shared__ int si[2][16];
    __shared__ __attribute__((aligned(16))) unsigned int s_next[4]; // [0]: the queue index this workgroup works on next
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    const int tid = threadIdx.x;
    if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u);
    __syncthreads();
    // The loop shape is lp_batch_kernel's (see the comment there): the top only READS the slot, one lane fetches the next
    // index in the middle of the body between two barriers, and the body ends with a barrier.
    for (;;) {
        const unsigned int k = __builtin_amdgcn_readfirstlane(s_next[0]);
        if (k >= (unsigned int)L.count) return;
        const int i = L.order[k];
        const NodeDesc *d = L.node + i;
        const LpDesc *rt = L.roots + d->root;
        const int w = rt->w, h0 = rt->h, n = w - 1, ncuts = d->ncuts, h = h0 + ncuts;
        const int pcols = small_pcols(n), lp = LDS ? small_lds_pitch(n) : pcols;
        const long long cut_lo = d->cut_lo, col0_off = d->col0_off, perm_off = d->perm_off;
        const double *root = L.root_tab + rt->tab_off;
        const int32_t *root_pos = L.root_pos + rt->perm_off, *root_var = L.root_var + rt->perm_off;
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
        // ---- applyCuts (src/branchAndCut.ts:22-61): the root, one row per cut, permutations extended by identity ----
        {
            const int Uc = wg_unit_lanes(pcols, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
            for (int r = cg0; r < h0; r += CG) {
                const double *src = root + (size_t)r * w + 1;
                for (int c = cu0; c < lp; c += Uc) mat[(size_t)r * lp + c] = c < n ? src[c] : 0.0;
            }
            for (int r = tid; r < h0; r += T) rhs[r] = root[(size_t)r * w];
            for (int q = 0; q < ncuts; q++) {
                const double sign = (double)L.cut_sign[cut_lo + q], value = L.cut_val[cut_lo + q];
                int v = L.cut_var[cut_lo + q];
                v = v < 0 ? 0 : (v >= w + h0 ? w + h0 - 1 : v); // (the host has refused such cuts)
                const int p = root_pos[v];
                double *dst = mat + (size_t)(h0 + q) * lp;
                if (p < w) { // non-basic at the root: sign * x <= sign * value   (:32-35)
                    for (int c = tid; c < lp; c += T) dst[c] = (c == p - 1) ? sign : 0.0;
                    if (tid == 0) rhs[h0 + q] = sign * value;
                } else { // basic in root row p - w: substitute that row   (:36-42)
                    const double *src = root + (size_t)(p - w) * w + 1;
                    for (int c = tid; c < lp; c += T) dst[c] = c < n ? -sign * src[c] : 0.0;
                    if (tid == 0) rhs[h0 + q] = sign * (value - src[-1]);
                }
            }
            for (int p = tid; p < w + h; p += T) { // :46-52
                pos[p] = p < w + h0 ? root_pos[p] : p;
                var[p] = p < w + h0 ? root_var[p] : p;
            }
        }
        __syncthreads();
        if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u); // (everybody read the slot a barrier ago; read again after the last one)

        int32_t *hist_l = CHECK ? L.hist + (size_t)blockIdx.x * 2 * L.hist_cap : nullptr;
        const WgResult out = wg_simplex<T, CHECK>(mat, rhs, pos, var, colbuf, prow, sk, si, w, n, lp, pcols, h,
                                                  wg_unit_lanes(pcols / 2, T), rt->precision, d->max_pivots, hist_l,
                                                  CHECK ? hist_l + L.hist_cap : nullptr, CHECK ? L.hist_cap : 0);
        __syncthreads();
        // (checkCycles, history full: no output but the status -- the host grows the history and reruns this node)
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
            L.height[i] = h;
            if (done) {
                L.result[i] = out.result;
                L.pivots[i] = out.pivots;
            }
        }
        __syncthreads(); // everybody is done with this node's tableau, and the next index is in its slot
    }
}
