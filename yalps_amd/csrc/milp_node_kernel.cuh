// milp_node_kernel.cuh -- branch-and-cut nodes of many roots of different shapes, one workgroup per node at a time
// Part of libyalps_milpbatch.so; included by milp_batch.hip inside its anonymous namespace (gfx950 only).
#pragma once
#include "lp_batch_kernel.cuh"

// ------------------------------------------------------------------------------------------
// milp_node_kernel: the work queue of wg_queue.cuh (one launch covers nodes of any mix of roots and shapes, handed out
// largest first from a device counter, no waiting between workgroups) around batch_kernel's applyCuts
// (src/branchAndCut.ts:22-61).  The roots are the optimal tableaux the root pass (lp_batch_kernel, kept tableaux) left on
// the device: row-major width x height with column 0 in front, permutations at the root's perm_off.  A node is its root
// plus one row per cut; it is solved by wg_simplex (wg_simplex.cuh) unchanged with the ROOT's precision and checkCycles and
// the node's pivot budget (the root's maxPivots, src/branchAndCut.ts:127, unless the host overrides it).
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

struct NodeLaunch : QueueLaunch {
    const LpDesc *roots;          // [roots]: w, h, tab_off, perm_off, precision of every root
    const double *root_tab;       // the roots' final matrices
    const int32_t *root_pos, *root_var;
    const NodeDesc *node;         // [nodes of the pass]
    const int32_t *cut_sign, *cut_var;
    const double *cut_val;
    int32_t *height;              // per node of the pass
};

// applyCuts (src/branchAndCut.ts:22-61): the root, one row per cut, permutations extended by identity
// (milp_tree_kernel.cuh's tree_fill is a copy of fill() below with the cuts read from a slot: a change here goes there too)
struct NodeJob : QueueJobBase {
    const NodeLaunch &L;
    const NodeDesc *d;
    const LpDesc *rt;
    const double *root;
    const int32_t *root_pos, *root_var;
    long long cut_lo;
    int h0, ncuts;
    __device__ __forceinline__ explicit NodeJob(const NodeLaunch &launch) : L(launch) {}
    __device__ __forceinline__ QueueItem item(int i) {
        d = L.node + i;
        rt = L.roots + d->root;
        h0 = rt->h;
        ncuts = d->ncuts;
        cut_lo = d->cut_lo;
        root = L.root_tab + rt->tab_off;
        root_pos = L.root_pos + rt->perm_off;
        root_var = L.root_var + rt->perm_off;
        return QueueItem{rt->w, h0 + ncuts, d->col0_off, d->perm_off, d->aux_hbm};
    }
    __device__ __forceinline__ double precision() const { return rt->precision; }
    __device__ __forceinline__ double max_pivots() const { return d->max_pivots; }
    __device__ __forceinline__ long long tab_off(int, const QueueItem &) const { return d->tab_off; }
    template <int T, bool LDS>
    __device__ __forceinline__ void fill(const QueueItem &it, double *mat, double *rhs, int32_t *pos, int32_t *var, int lp) const {
        const int tid = threadIdx.x, w = it.w, h = it.h, n = w - 1;
        const int Uc = wg_unit_lanes(small_pcols(n), T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
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
    __device__ __forceinline__ void record(int i, const QueueItem &it) const { L.height[i] = it.h; }
};

template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_node_kernel(NodeLaunch L) {
    wg_queue<T, CHECK, LDS>(L, NodeJob(L));
}
