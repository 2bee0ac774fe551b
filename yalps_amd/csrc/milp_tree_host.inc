// milp_tree_host.inc -- host side of milp_tree_kernel: the tree pass, its arenas and its reruns.  Included inside the anonymous
// namespace of milp_tree.hip (libyalps_milptree.so) and milp_dense.hip (libyalps_milpdense.so) after milp_tree_kernel.cuh and
// wg_queue_host.inc: one text, two libraries, each with its own root pass.  What a root pass hands over is TreeRoots; what the
// tree pass owns is TreePass.
const KernelTable<TreeLaunch> kTreeKernels = QUEUE_KERNEL_TABLE(milp_tree_kernel);
constexpr int ARENA_FIRST = 128, ARENA_MAX = 1 << 16;
constexpr long long ARENA_BYTES = 1ll << 31; // bound on the arena buffer of a pass that runs trees again (grid x stride)
constexpr int TREE_TIMEDOUT = 4, TREE_OVERFLOW = 5; // every library's YALPS_*_TIMEDOUT / YALPS_*_OVERFLOW
static_assert(MT_TIMEDOUT == TREE_TIMEDOUT && MT_HIST_FULL == WG_HISTORY_FULL && MT_OPTIMAL == YALPS_OPTIMAL &&
                  MT_INFEASIBLE == YALPS_INFEASIBLE && sizeof(MtState) % sizeof(double) == 0 && NCLASS == 5,
              "milp_tree_rules.cuh");

// the root pass as the tree pass reads it: tree i is root i
struct TreeRoots {
    const QueueDevice *dev;       // the card, the stream, the events, the class table
    const LpDesc *host, *device;  // [trees] the roots' shapes and offsets, on both sides
    const QueueBufs *q;           // the kept root tableaux, column 0, permutations, status, result
};

struct TreePass {
    QueueBufs q;
    DevBuf tdesc, ints, globals, arena, nodebuf, d_used, d_best_h, d_trace;
    int arena_first = ARENA_FIRST, arena_max = ARENA_MAX, grid = 0;
    long long arena_bytes = ARENA_BYTES;
    // the last solve
    std::vector<TreeDesc> trees;
    int32_t trace_cap = 0;
    // info
    std::string lines;
    std::vector<int32_t> rerun_ids;
    int64_t launches = 0, overflows = 0;
    double gpu_ms = 0.0;
};
void release(TreePass &t) {
    release(t.q);
    release({&t.tdesc, &t.ints, &t.globals, &t.arena, &t.nodebuf, &t.d_used, &t.d_best_h, &t.d_trace});
}

// The tree pass: passes over the trees left until none ends with an internal code.  One pass is the launches of
// plan_launches -- a tree counts as its largest possible node -- over the workgroups' arenas; a tree whose arena or whose
// node's history was too short runs again, alone with the others of its kind, from its root with four times that room.
// check(i): checkCycles of tree i.  lib: "yalps_milptree", for the messages.
template <class Check>
int trees_impl(TreePass *b, const TreeRoots &roots, size_t n, Check check, const std::string &lib) {
    hipStream_t s = roots.dev->stream;
    const std::vector<TreeDesc> &D = b->trees;
    const LpDesc *R = roots.host;
    QueueDevice dev = *roots.dev; // (the class table as this handle runs it; the stream and the events are the root pass's)
    if (b->grid > 0) {
        dev.num_cus = 1;
        for (int k = 0; k < NCLASS; k++) dev.per_cu[k] = b->grid;
    }
    std::vector<int32_t> todo(n);
    for (size_t i = 0; i < n; i++) todo[i] = (int32_t)i;
    std::vector<Launch> launches;
    std::vector<int32_t> overflowed;
    long long hist_cap = b->q.hist_first, arena_cap = std::max(2, b->arena_first);
    bool grew = false; // this pass runs with an arena four times the last one's
    // the trees of `todo` that ended with a full arena get the public status and leave the pass; the arena shrinks back
    auto give_up_arena = [&]() {
        std::vector<int32_t> keep;
        for (int32_t i : todo) (b->q.h_status[(size_t)i] == MT_ARENA_FULL ? overflowed : keep).push_back(i);
        todo.swap(keep);
        arena_cap /= 4, grew = false;
    };
    for (int pass = 0; !todo.empty(); pass++) {
        TreeGlobals G{};
        size_t arena_doubles = 0, node_doubles = 0;
        for (;;) { // the pass's launches and what they need; a grown arena beyond the byte bound is given up like one above the cap
            if (int rc = plan_launches(dev, b->q, todo, [&](int32_t i, int *w, int *h) {
                    return *w = R[(size_t)i].w, *h = R[(size_t)i].h + 2 * D[(size_t)i].nints, check(i);
                }, hist_cap, launches))
                return rc;
            G = TreeGlobals{};
            for (int32_t i : todo) {
                const TreeDesc &d = D[(size_t)i];
                const LpDesc &r = R[(size_t)i];
                G.arena_stride[d.cls] = std::max<long long>(G.arena_stride[d.cls], (long long)mt_arena_doubles((int32_t)arena_cap, d.maxcuts));
                if (d.cls == HBM_CLASS) {
                    const long long hmax = r.h + 2 * d.nints;
                    G.nodebuf_stride = std::max(G.nodebuf_stride, ((hmax + 1) & ~1ll) + ((r.w + hmax + 1) & ~1ll));
                }
            }
            arena_doubles = node_doubles = 0;
            for (const Launch &L : launches) {
                if (!find_form(kTreeKernels, L.lanes, L.check, L.cls != HBM_CLASS))
                    return fail(YALPS_E_ARG, lib + ": no kernel of " + std::to_string(L.lanes) + " lanes");
                arena_doubles = std::max(arena_doubles, (size_t)L.grid * (size_t)G.arena_stride[L.cls]);
                if (L.cls == HBM_CLASS) node_doubles = std::max(node_doubles, (size_t)L.grid * (size_t)G.nodebuf_stride);
            }
            if (!grew || sizeof(double) * arena_doubles <= (size_t)b->arena_bytes) break;
            give_up_arena();
            if (todo.empty()) break;
        }
        if (todo.empty()) break;
        if (pass > 0) b->rerun_ids.insert(b->rerun_ids.end(), todo.begin(), todo.end());
        if (int rc = ensure(b->arena, sizeof(double) * arena_doubles)) return rc;
        if (int rc = ensure(b->nodebuf, sizeof(double) * node_doubles)) return rc;
        G.roots = roots.device;
        G.root_tab = roots.q->tab.as<const double>();
        G.root_col0 = roots.q->col0.as<const double>();
        G.root_result = roots.q->result.as<const double>();
        G.root_pos = roots.q->pos.as<const int32_t>();
        G.root_var = roots.q->var.as<const int32_t>();
        G.root_status = roots.q->status.as<const int32_t>();
        G.tree = b->tdesc.as<const TreeDesc>();
        G.ints = b->ints.as<const int32_t>();
        G.status = b->q.status.as<int32_t>();
        G.result = b->q.result.as<double>();
        G.used = b->d_used.as<long long>();
        G.pivots = b->q.pivots.as<long long>();
        G.best_h = b->d_best_h.as<int32_t>();
        G.col0 = b->q.col0.as<double>();
        G.pos = b->q.pos.as<int32_t>();
        G.var = b->q.var.as<int32_t>();
        G.trace = b->trace_cap > 0 ? b->d_trace.as<double>() : nullptr;
        G.arena = b->arena.as<double>();
        G.nodebuf = b->nodebuf.as<double>();
        G.trace_cap = b->trace_cap;
        G.arena_cap = (int32_t)arena_cap;
        std::vector<TreeGlobals> per(launches.size(), G); // (one per launch: its part of the order, its counter, its stride)
        for (size_t nl = 0; nl < launches.size(); nl++) {
            const Launch &L = launches[nl];
            per[nl].order = b->q.order.as<const int32_t>() + L.at;
            per[nl].count = (int32_t)L.items.size();
            per[nl].counter = b->q.counters.as<unsigned int>() + nl;
            per[nl].ws = b->q.ws.as<double>();
            per[nl].ws_stride = (long long)L.stride;
            per[nl].hist = b->q.hist.as<int32_t>();
            per[nl].hist_cap = hist_cap;
        }
        if (int rc = ensure(b->globals, sizeof(TreeGlobals) * per.size())) return rc;
        HIP_TRY(hipMemcpyAsync(b->globals.p, per.data(), sizeof(TreeGlobals) * per.size(), hipMemcpyHostToDevice, s));
        HIP_TRY(hipStreamSynchronize(s)); // (`per` is on this frame)
        HIP_TRY(hipEventRecord(dev.ev0, s));
        for (size_t nl = 0; nl < launches.size(); nl++) {
            const Launch &L = launches[nl];
            const KernelForm<TreeLaunch> *form = find_form(kTreeKernels, L.lanes, L.check, L.cls != HBM_CLASS);
            TreeLaunch a{b->globals.as<const TreeGlobals>() + nl};
            form->fn<<<dim3(L.grid), dim3(form->lanes), L.shmem, s>>>(a);
            HIP_TRY(hipGetLastError());
            char line[288];
            std::snprintf(line, sizeof line, "launch=%lld pass=%d kernel=%s class=%d trees=%zu grid=%d lds=%zu hist_cap=%lld arena=%lld\n",
                          (long long)b->launches++, pass, form_name(kTreeKernels, *form).c_str(), L.cls, L.items.size(), L.grid, L.shmem,
                          L.check ? hist_cap : 0ll, arena_cap);
            if (b->lines.size() < ((size_t)1 << 20)) b->lines += line;
        }
        HIP_TRY(hipEventRecord(dev.ev1, s));
        HIP_TRY(hipMemcpyAsync(b->q.h_status.data(), b->q.status.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        float ms = 0.f;
        HIP_TRY(hipEventElapsedTime(&ms, dev.ev0, dev.ev1));
        b->gpu_ms += ms;
        std::vector<int32_t> again;
        bool arena_full = false, hist_full = false;
        for (int32_t i : todo) {
            const int32_t st = b->q.h_status[(size_t)i];
            if (st == MT_ARENA_FULL)
                arena_full = true, again.push_back(i);
            else if (st == MT_HIST_FULL)
                hist_full = true, again.push_back(i);
            else if (st < 0 || st > TREE_TIMEDOUT)
                return fail(YALPS_E_DEVICE, "milp_tree_kernel did not report a result for tree " + std::to_string(i));
        }
        if (hist_full) hist_cap *= 4;
        if (hist_full && hist_cap > (1ll << 28)) return fail(YALPS_E_NOMEM, lib + "_solve: checkCycles history beyond 2^28 pivots");
        todo.swap(again);
        grew = arena_full;
        if (arena_full) arena_cap *= 4;
        if (arena_full && arena_cap > b->arena_max) give_up_arena(); // above the cap
    }
    for (int32_t i : overflowed) b->q.h_status[(size_t)i] = TREE_OVERFLOW; // (the device's word for it is internal)
    b->overflows = (int64_t)overflowed.size();
    return 0;
}

// the first `cnt` records of one tree's trace (tree_step's layout) as yalps_*_trace hands them out; h0: the root's height
void tree_trace_out(const double *trace, int32_t maxcuts, int32_t cnt, int32_t h0, double *eval, int32_t *status, double *result,
                    int64_t *pivots, int32_t *height, int32_t *cut_sign, int32_t *cut_var, double *cut_val) {
    size_t c = 0;
    for (int32_t k = 0; k < cnt; k++) {
        const double *e = trace + (size_t)k * (4 + 2 * (size_t)maxcuts);
        int32_t sh[2];
        int64_t piv;
        std::memcpy(&piv, e + 2, sizeof piv);
        std::memcpy(sh, e + 3, sizeof sh);
        if (eval) eval[k] = e[0];
        if (result) result[k] = e[1];
        if (pivots) pivots[k] = piv;
        if (status) status[k] = sh[0];
        if (height) height[k] = sh[1];
        for (int32_t q = 0; q < sh[1] - h0; q++, c++) {
            int32_t sv[2];
            std::memcpy(sv, e + 5 + 2 * q, sizeof sv);
            if (cut_sign) cut_sign[c] = sv[0];
            if (cut_var) cut_var[c] = sv[1];
            if (cut_val) cut_val[c] = e[4 + 2 * q];
        }
    }
}
