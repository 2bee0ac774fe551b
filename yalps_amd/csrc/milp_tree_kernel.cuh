// milp_tree_kernel.cuh -- whole branch-and-cut trees of many roots of different shapes, one workgroup per tree at a time
// Part of libyalps_milptree.so; included by milp_tree.hip inside its anonymous namespace (gfx950 only), after
// milp_tree_rules.cuh (file scope) and lp_batch_kernel.cuh.
#pragma once

// ------------------------------------------------------------------------------------------
// milp_tree_kernel: wg_queue's outer loop (trees handed out largest first from a device counter, no waiting between
// workgroups) around the search loop of src/branchAndCut.ts:89-176.  Per tree: the rules of milp_tree_rules.cuh on the
// workgroup's arena in HBM, run by ONE lane in tree_step; per node: milp_node_kernel's applyCuts from the resident root with
// the cuts read from the node's slot, then wg_simplex unchanged with the root's precision, maxPivots and checkCycles.
// A tree's class, LDS bytes and aux form are those of its largest possible node (h0 + 2 * n_integers rows); a node's layout
// pointers follow its own height.
//
// Uniformity (wg_queue.cuh, the hang of a one-lane block next to a back edge): every decision that steers a loop -- the next
// node exists, its height, its slot, it is an incumbent, the next tree's queue index -- is written by lane 0 INSIDE the
// not-inlined tree_step into a padded LDS slot, between two barriers, and read by every lane with readfirstlane after the
// barrier.  The kernel body holds no per-lane branch at all.
// ------------------------------------------------------------------------------------------
struct TreeDesc {
    int32_t nints, maxcuts;       // maxcuts = max(1, 2 * nints): the cuts of a slot
    long long ints_off;           // its integer variables at ints[ints_off .. + nints)
    double sign, tolerance, max_iter;
    int32_t timedout, cls;        // timeout <= 0; size class of its largest node
    long long col0_off, perm_off; // the best tableau's column 0 / permutations (room for the largest node)
    long long trace_off;          // doubles into the trace
    int32_t aux_hbm, pad_;        // HBM form: colbuf / prow behind the tableau (of the largest node)
};

// What a launch works on, in device memory (written once per pass, one per launch).  The kernel's only argument is the pointer
// to it: what is read from memory is read again after every barrier, while kernel arguments are loaded once and held in
// scalar registers through wg_simplex, where <1024,check> has none to spare.
struct TreeGlobals {
    const int32_t *order;         // [count] tree indices of this launch, largest first
    unsigned int *counter;        // next entry of `order` to hand out (zeroed before the launch)
    double *ws;                   // HBM form: [grid][ws_stride]
    int32_t *hist;                // checkCycles: [grid][2][hist_cap] pivot history of the node a workgroup is solving
    long long ws_stride, hist_cap;
    int32_t count, pad_;
    const LpDesc *roots;          // the root pass: tree i is root i
    const double *root_tab, *root_col0, *root_result;
    const int32_t *root_pos, *root_var, *root_status;
    const TreeDesc *tree;
    const int32_t *ints;
    int32_t *status;              // per tree: YALPS_*, MT_TIMEDOUT, or MT_ARENA_FULL / MT_HIST_FULL (the host reruns it)
    double *result;
    long long *used, *pivots;
    int32_t *best_h;              // 0: no incumbent, the best tableau is the root
    double *col0;
    int32_t *pos, *var;
    double *trace;                // nullptr: off
    double *arena;                // [grid][arena_stride[class]]
    double *nodebuf;              // HBM form: [grid][nodebuf_stride] column 0 and permutations of the node at work
    long long arena_stride[5], nodebuf_stride;
    int32_t trace_cap, arena_cap;
};

struct TreeLaunch {
    const TreeGlobals *g;
};

constexpr int TREE_FIRST = -1, TREE_BEGIN = 0, TREE_CONSUME = 1;

// The step between two nodes, lane 0's (tid: the caller's threadIdx.x).  TREE_FIRST only takes the workgroup's first queue
// index.  TREE_BEGIN takes the next one into s_next[0] (everybody read it a barrier ago), leaves i in s_next[2] and starts
// tree i on the solved root; TREE_CONSUME feeds the solved node (column 0 and positionOfVariable read where its tableau
// lies) to the search.  Both then pop the next node or finish the tree, and leave the decisions in dec[0..3]: node exists,
// its height, its slot, the height of the node just solved where it is the incumbent (else 0).  A function of its own, not
// inlined, as lp_sens_kernel's epilogue and for its reason (inlined, it cost <1024,check> twenty spilled registers), and so
// that its one-lane block cannot be threaded into the loops around it.
__device__ __attribute__((noinline)) void tree_step(const TreeGlobals *g, int i, double *arena, int mode, const double *rhs,
                                                    const int32_t *pos, int st, double res, long long piv, int h, int *dec,
                                                    unsigned int *s_next, int tid) {
    if (tid != 0) return;
    if (mode == TREE_FIRST) {
        s_next[0] = atomicAdd(g->counter, 1u);
        return;
    }
    const TreeDesc *d = g->tree + i;
    const LpDesc *rt = g->roots + i;
    const MtTree T = {rt->w, d->nints, g->ints + d->ints_off, d->sign, rt->precision, d->tolerance, d->max_iter, d->timedout};
    const MtArena A = mt_arena_bind(arena, g->arena_cap, d->maxcuts);
    MtState &S = *A.state;
    int incumbent = 0;
    if (mode == TREE_BEGIN) {
        s_next[0] = atomicAdd(g->counter, 1u);
        s_next[2] = (unsigned int)i;
        mt_begin(T, A, g->root_status[i], g->root_result[i], g->root_col0 + rt->col0_off, g->root_pos + rt->perm_off);
    } else if (st == WG_HISTORY_FULL) {
        mt_finish(A, MT_HIST_FULL, NAN);
    } else {
        if (g->trace && S.used < g->trace_cap) { // the node as it was popped, and what simplex() made of it
            double *e = g->trace + d->trace_off + (size_t)S.used * (4 + 2 * (size_t)d->maxcuts);
            const int ncuts = A.slot_n[S.cur_slot];
            e[0] = S.cur_eval;
            e[1] = res;
            reinterpret_cast<long long *>(e)[2] = piv;
            reinterpret_cast<int32_t *>(e)[6] = st;
            reinterpret_cast<int32_t *>(e)[7] = h;
            for (int q = 0; q < ncuts; q++) {
                const size_t at = (size_t)S.cur_slot * d->maxcuts + q;
                e[4 + 2 * q] = A.cut_val[at];
                reinterpret_cast<int32_t *>(e)[2 * (5 + 2 * q)] = A.cut_sv[2 * at];
                reinterpret_cast<int32_t *>(e)[2 * (5 + 2 * q) + 1] = A.cut_sv[2 * at + 1];
            }
        }
        S.pivots += piv;
        incumbent = mt_consume(T, A, st, res, rhs, pos, h) == MT_INCUMBENT;
    }
    const int more = mt_next(T, A);
    dec[0] = more;
    dec[1] = more ? rt->h + A.slot_n[S.cur_slot] : 0;
    dec[2] = more ? S.cur_slot : 0;
    dec[3] = incumbent ? h : 0;
    if (!more) {
        g->status[i] = S.status;
        g->result[i] = S.result;
        g->used[i] = S.used;
        g->pivots[i] = S.pivots;
        g->best_h[i] = S.best_height;
    }
}

// NodeJob::fill's applyCuts (src/branchAndCut.ts:22-61) with the cuts of a slot: the root, one row per cut, permutations
// extended by identity.  Every lane calls it; it has no barrier.  Not inlined either: inlined, <1024,check> in the HBM form
// spilled two registers of wg_simplex's cycle check to scratch (in the LDS form its stores are flat ones for that).
// A SECOND COPY of applyCuts: the loops below are NodeJob::fill's (milp_node_kernel.cuh) line for line, only the cuts come from
// elsewhere; that one stays as it is so that milp_node_kernel's code object does not change.  A change to either goes into both.
template <int T>
__device__ __attribute__((noinline)) void tree_fill(const double *root, const int32_t *root_pos, const int32_t *root_var, const int32_t *cut_sv,
                                          const double *cut_val, int w, int h0, int ncuts, double *mat, double *rhs, int32_t *pos,
                                          int32_t *var, int lp) {
    const int tid = threadIdx.x, h = h0 + ncuts, n = w - 1;
    const int Uc = wg_unit_lanes(small_pcols(n), T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
    for (int r = cg0; r < h0; r += CG) {
        const double *src = root + (size_t)r * w + 1;
        for (int c = cu0; c < lp; c += Uc) mat[(size_t)r * lp + c] = c < n ? src[c] : 0.0;
    }
    for (int r = tid; r < h0; r += T) rhs[r] = root[(size_t)r * w];
    for (int q = 0; q < ncuts; q++) {
        const double sign = (double)cut_sv[2 * q], value = cut_val[q];
        int v = cut_sv[2 * q + 1];
        v = v < 0 ? 0 : (v >= w + h0 ? w + h0 - 1 : v); // (the search only cuts on the model's integer variables)
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

// the incumbent's column 0 and permutations to the tree's output slice (not inlined, as tree_step)
template <int T>
__device__ __attribute__((noinline)) void tree_keep(const double *rhs, const int32_t *pos, const int32_t *var, double *col0, int32_t *opos,
                                                    int32_t *ovar, int h, int np, int tid) {
    for (int r = tid; r < h; r += T) col0[r] = rhs[r];
    for (int p = tid; p < np; p += T) {
        opos[p] = pos[p];
        ovar[p] = var[p];
    }
}

// where a node of h rows of tree i lies: wg_queue's layout, in the HBM form with column 0 and the permutations in the
// workgroup's node buffer (a node is nobody's output)
struct TreeNodeAt {
    double *mat, *rhs, *colbuf, *prow;
    int32_t *pos, *var;
    int w, h0, lp;
};
template <bool LDS>
__device__ __forceinline__ TreeNodeAt tree_node_at(const TreeGlobals *g, int i, int h, double *sh_dyn) {
    const TreeDesc *d = g->tree + i;
    const LpDesc *rt = g->roots + i;
    TreeNodeAt at;
    const int w = rt->w, n = w - 1;
    at.w = w;
    at.h0 = rt->h;
    at.lp = LDS ? small_lds_pitch(n) : small_pcols(n);
    if (LDS) {
        at.mat = sh_dyn;
        at.rhs = at.mat + (size_t)h * at.lp;
        at.colbuf = at.rhs + h;
        at.prow = at.colbuf + h;
        at.pos = reinterpret_cast<int32_t *>(at.prow + at.lp);
        at.var = at.pos + ((w + h + 1) & ~1);
    } else {
        const int hmax = rt->h + 2 * d->nints;
        at.mat = g->ws + (size_t)blockIdx.x * g->ws_stride;
        at.rhs = g->nodebuf + (size_t)blockIdx.x * g->nodebuf_stride;
        at.pos = reinterpret_cast<int32_t *>(at.rhs + ((hmax + 1) & ~1));
        at.var = at.pos + ((w + hmax + 1) & ~1);
        at.prow = d->aux_hbm ? at.mat + (size_t)h * at.lp : sh_dyn;
        at.colbuf = at.prow + at.lp;
    }
    return at;
}

// Nothing of a tree is kept in registers across wg_simplex: the tree's index and the decisions lie in LDS, and each part of
// the node loop -- fill and solve, the step, the incumbent's copy -- reads them again after its barrier and derives what it
// needs (<1024,check> in the HBM form is a few registers under the 128 a workgroup of 1024 lanes may use).
template <int T, bool CHECK, bool LDS>
__global__ __launch_bounds__(T) void milp_tree_kernel(TreeLaunch L) {
    __shared__ double sk[2][16];
    __shared__ int si[2][16];
    __shared__ __attribute__((aligned(16))) unsigned int s_next[4]; // [0]: the queue index this workgroup works on next; [2]: the tree at work
    __shared__ __attribute__((aligned(16))) int s_dec[4];           // tree_step's decisions
    extern __shared__ __attribute__((aligned(16))) double sh_dyn[];
    const int tid = threadIdx.x;
    tree_step(L.g, 0, nullptr, TREE_FIRST, nullptr, nullptr, 0, 0.0, 0, 0, s_dec, s_next, tid);
    __syncthreads();
    for (;;) {
        const unsigned int k = __builtin_amdgcn_readfirstlane(s_next[0]);
        if (k >= (unsigned int)L.g->count) return;
        __syncthreads(); // (everybody has read the index: tree_step puts the next one in its place)
        {
            const TreeGlobals *g = L.g;
            const int i = g->order[k];
            double *arena = g->arena + (size_t)blockIdx.x * g->arena_stride[g->tree[i].cls];
            tree_step(g, i, arena, TREE_BEGIN, nullptr, nullptr, 0, 0.0, 0, 0, s_dec, s_next, tid);
        }
        __syncthreads();
        for (;;) {
            if (!__builtin_amdgcn_readfirstlane(s_dec[0])) break;
            WgResult out;
            {
                const TreeGlobals *g = L.g;
                const int i = __builtin_amdgcn_readfirstlane(s_next[2]), h = __builtin_amdgcn_readfirstlane(s_dec[1]);
                const int slot = __builtin_amdgcn_readfirstlane(s_dec[2]);
                const TreeDesc *d = g->tree + i;
                const LpDesc *rt = g->roots + i;
                const TreeNodeAt at = tree_node_at<LDS>(g, i, h, sh_dyn);
                const MtArena A = mt_arena_bind(g->arena + (size_t)blockIdx.x * g->arena_stride[d->cls], g->arena_cap, d->maxcuts);
                const int w = at.w, n = w - 1, pcols = small_pcols(n);
                tree_fill<T>(g->root_tab + rt->tab_off, g->root_pos + rt->perm_off, g->root_var + rt->perm_off,
                             A.cut_sv + 2 * (size_t)slot * d->maxcuts, A.cut_val + (size_t)slot * d->maxcuts, w, at.h0, h - at.h0, at.mat,
                             at.rhs, at.pos, at.var, at.lp);
                __syncthreads();
                const long long hist_cap = CHECK ? g->hist_cap : 0;
                int32_t *hist_l = CHECK ? g->hist + (size_t)blockIdx.x * 2 * hist_cap : nullptr;
                out = wg_simplex<T, CHECK>(at.mat, at.rhs, at.pos, at.var, at.colbuf, at.prow, sk, si, w, n, at.lp, pcols, h,
                                           wg_unit_lanes(pcols / 2, T), rt->precision, rt->max_pivots, hist_l,
                                           CHECK ? hist_l + hist_cap : nullptr, hist_cap);
            }
            __syncthreads();
            {
                // Only lane 0 of wave 0 uses `h` and `at` here (inside tree_step), and it reads s_dec[1] before it writes the next
                // node's decisions there.  Another wave may read s_dec[1] while that write is under way: its value is unused (the
                // pointers of `at` are computed, never followed), and every wave reads the slot again after the next barrier.
                const TreeGlobals *g = L.g;
                const int i = __builtin_amdgcn_readfirstlane(s_next[2]), h = __builtin_amdgcn_readfirstlane(s_dec[1]);
                const TreeNodeAt at = tree_node_at<LDS>(g, i, h, sh_dyn);
                double *arena = g->arena + (size_t)blockIdx.x * g->arena_stride[g->tree[i].cls];
                tree_step(g, i, arena, TREE_CONSUME, at.rhs, at.pos, out.status, out.result, out.pivots, h, s_dec, s_next, tid);
            }
            __syncthreads();
            const int best_h = __builtin_amdgcn_readfirstlane(s_dec[3]);
            if (best_h) { // the node just solved is the incumbent: what solution() reads of it
                const TreeGlobals *g = L.g;
                const int i = __builtin_amdgcn_readfirstlane(s_next[2]);
                const TreeDesc *d = g->tree + i;
                const TreeNodeAt at = tree_node_at<LDS>(g, i, best_h, sh_dyn);
                tree_keep<T>(at.rhs, at.pos, at.var, g->col0 + d->col0_off, g->pos + d->perm_off, g->var + d->perm_off, best_h, at.w + best_h, tid);
            }
            __syncthreads(); // the node's tableau is free, and the decisions about the next one are in their slot
        }
        __syncthreads(); // everybody has read this tree's decisions; the next index is in its slot
    }
}
