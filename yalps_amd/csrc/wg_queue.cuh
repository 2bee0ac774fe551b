// wg_queue.cuh -- the work queue every batch kernel runs: a device counter hands items to workgroups, wg_simplex solves each
// Included by lp_batch_kernel.cuh, lp_sens_kernel.cuh, lp_variants_kernel.cuh and milp_node_kernel.cuh (gfx950 only).
#pragma once

// ------------------------------------------------------------------------------------------
// A launch covers items (LPs, variants, branch-and-cut nodes) of any mix of shapes.  Workgroups do not own an item: each
// takes the next index of the launch's order (largest first) from a device counter until the counter passes the count, so
// items whose pivot counts differ by orders of magnitude still fill the chip.  There is no waiting between workgroups of
// any kind: a workgroup that is not resident yet simply takes its first index later.
// Per item: the job writes the initial tableau, then wg_simplex (wg_simplex.cuh) unchanged, then the outputs.
// LDS = true: tableau, rhs, colbuf, prow and both permutations in LDS, small_kernel's layout (small_lds_pitch).
// LDS = false: the tableau in this workgroup's workspace in HBM (L2-resident while it is worked on), column 0 and the
// permutations directly at the item's output offsets, colbuf / prow in LDS where they fit the launch's allocation.
// ------------------------------------------------------------------------------------------

// What every queue kernel's launch begins with.  The order of the fields is deliberate: do not rearrange them without building
// all four libraries through build.check_register_budgets.  hipcc loads the kernel arguments in 16-dword runs, and with the
// three per-item records ahead of col0 .. hist_cap (12 of the 24 orders of these four groups) its register allocator first
// spilled such a run in lp_sens_kernel<256, false, true>, then split it instead, and left the 64-byte slot in the frame:
// no instruction touches it, but the kernel then asks for scratch and the build refuses it.
struct QueueLaunch {
    const int32_t *order;         // [count] item indices of this launch, largest first
    int32_t count;
    unsigned int *counter;        // next entry of `order` to hand out (zeroed before the launch)
    double *col0;
    int32_t *pos, *var;
    double *tab;                  // nullptr unless keep_tableaux
    double *ws;                   // HBM form: [grid][ws_stride]
    long long ws_stride;
    int32_t *hist;                // checkCycles: [grid][2][hist_cap] pivot history of the item a workgroup is solving
    long long hist_cap;
    int32_t *status;              // per item
    double *result;
    long long *pivots;
};

// what a job tells the queue about item i
struct QueueItem {
    int32_t w, h;
    long long col0_off;           // column 0 at col0[col0_off .. + h)
    long long perm_off;           // the permutations at pos / var[perm_off .. + w + h)
    int32_t aux_hbm;              // HBM form: colbuf / prow behind the tableau in the workspace (too long for the LDS block)
};

// A job is an object with
//   QueueItem item(int i)                                   shape and offsets of item i (it may keep what fill needs)
//   precision(), max_pivots()                               its options, read when the solve begins
//   tab_off(i, it)                                          keep_tableaux: the final matrix, row-major w * h, at tab[tab_off ..)
// (what is read early stays in registers through the solve: only what the layout needs is)
//   fill<T, LDS>(it, mat, rhs, pos, var, lp)                the initial tableau and permutations, every lane, barriers of its own
//   record(i, it)                                           one lane, next to the status: any further per-item record
//   after<T>(it, status, mat, rhs, lp)                      every lane, between the outputs and the last barrier
// The dynamic LDS block holds the tableau and prow, which wg_simplex sweeps 16 bytes at a time: it must start on a 16-byte
// boundary, so the static objects in front of it add up to a multiple of 16 (the queue slot is padded to 16 bytes;
// build.check_register_budgets refuses a library whose kernels' static LDS is not).
template <int T, bool CHECK, bool LDS, class Job>
__device__ __forceinline__ void wg_queue(const QueueLaunch &L, Job job) {
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
    // it and the kernel never ended).  A job's `after` keeps to that: it sits between the outputs and the last barrier, under
    // conditions every lane shares.
    for (;;) {
        const unsigned int k = __builtin_amdgcn_readfirstlane(s_next[0]);
        if (k >= (unsigned int)L.count) return;
        const int i = L.order[k];
        const QueueItem it = job.item(i);
        const int w = it.w, h = it.h, n = w - 1;
        const int pcols = small_pcols(n), lp = LDS ? small_lds_pitch(n) : pcols;
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
            rhs = L.col0 + it.col0_off;
            pos = L.pos + it.perm_off;
            var = L.var + it.perm_off;
            prow = it.aux_hbm ? mat + (size_t)h * lp : sh_dyn;
            colbuf = prow + lp;
        }
        job.template fill<T, LDS>(it, mat, rhs, pos, var, lp);
        __syncthreads();
        if (tid == 0) s_next[0] = atomicAdd(L.counter, 1u); // (everybody read the slot at least a barrier ago; read again after the last one)

        int32_t *hist_l = CHECK ? L.hist + (size_t)blockIdx.x * 2 * L.hist_cap : nullptr;
        const WgResult out = wg_simplex<T, CHECK>(mat, rhs, pos, var, colbuf, prow, sk, si, w, n, lp, pcols, h,
                                                  wg_unit_lanes(pcols / 2, T), job.precision(), job.max_pivots(), hist_l,
                                                  CHECK ? hist_l + L.hist_cap : nullptr, CHECK ? L.hist_cap : 0);
        __syncthreads();
        // (checkCycles, history full: no output but the status -- the host grows the history and reruns this item)
        const bool done = !(CHECK && out.status == WG_HISTORY_FULL);
        if (LDS && done) {
            double *col0 = L.col0 + it.col0_off;
            for (int r = tid; r < h; r += T) col0[r] = rhs[r];
            int32_t *opos = L.pos + it.perm_off, *ovar = L.var + it.perm_off;
            for (int p = tid; p < w + h; p += T) {
                opos[p] = pos[p];
                ovar[p] = var[p];
            }
        }
        if (L.tab && done) { // the whole final matrix in the reference's layout (src/tableau.ts:9-21)
            double *tab = L.tab + job.tab_off(i, it);
            const int Uc = wg_unit_lanes(w, T), cu0 = tid % Uc, cg0 = tid / Uc, CG = T / Uc;
            for (int r = cg0; r < h; r += CG) {
                const double *src = mat + (size_t)r * lp;
                double *dst = tab + (size_t)r * w;
                for (int c = cu0; c < w; c += Uc) dst[c] = c == 0 ? rhs[r] : src[c - 1];
            }
        }
        if (tid == T - 1) {
            L.status[i] = out.status;
            job.record(i, it);
            if (done) {
                L.result[i] = out.result;
                L.pivots[i] = out.pivots;
            }
        }
        // (last: by now only the tableau itself is still needed, which keeps an epilogue's registers off the solve's)
        job.template after<T>(it, out.status, mat, rhs, lp);
        __syncthreads(); // everybody is done with this item's tableau, and the next index is in its slot
    }
}

// a job without a further record or an epilogue
struct QueueJobBase {
    __device__ __forceinline__ void record(int, const QueueItem &) const {}
    template <int T>
    __device__ __forceinline__ void after(const QueueItem &, int, const double *, const double *, int) const {}
};
