// milp_batch.hip -- libyalps_milpbatch.so: a batch of independent MILPs in one call (include/yalps_milpbatch.h)
// The root pass is libyalps_lpbatch.so's host code and kernels (lp_batch_host.inc, lp_batch_kernel.cuh) with kept tableaux,
// compiled again here; the node pass is milp_node_kernel on the same passes (wg_queue_host.inc); the search rules are
// milp_search.inc, shared with yalps_milp_f64.
// A library of its own: nothing here is linked into libyalps_hip.so or libyalps_lpbatch.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <chrono>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <functional>
#include <map>
#include <set>
#include <string>
#include <vector>

#include "../../include/yalps_lpbatch.h"
#include "../../include/yalps_milpbatch.h"

#pragma clang fp contract(off)

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "milp_node_kernel.cuh"
#include "wg_queue_host.inc"
#include "lp_batch_host.inc"

static_assert(YALPS_MILPBATCH_MAX_BYTES == QUEUE_MAX_BYTES, "include/yalps_milpbatch.h");
const KernelTable<NodeLaunch> kNodeKernels = QUEUE_KERNEL_TABLE(milp_node_kernel);
} // namespace

#include "lp_batch_lib.inc"
#include "milp_search.inc"

namespace {
// one model of the whole solve / of the host-only search
struct Tree {
    int32_t w = 0, h = 0, nints = 0;
    const int32_t *ints = nullptr;
    double sign = 1.0, precision = 1e-8, tolerance = 0.0, timeout = INFINITY, max_iter = 32768.0;
    // search state (src/branchAndCut.ts:89-176)
    std::vector<MilpBranch> branches;
    std::map<MilpCuts, MilpEval> cache; // results of nodes evaluated ahead of their turn
    MilpView best;
    MilpBranch pending;                 // popped, waiting for its result
    bool has_pending = false, finished = false, timedout = false, found = false;
    double threshold = 0.0, stop_time = 0.0, best_eval = INFINITY, iter = 0.0;
    int64_t used = 0, evaluated = 0;
    int32_t status = YALPS_CYCLED;
    double result = NAN;
};

using EvalFn = std::function<int(const std::vector<int32_t> &model, const std::vector<int64_t> &off, const std::vector<int32_t> &sg,
                                 const std::vector<int32_t> &vr, const std::vector<double> &vl, std::vector<MilpEval> &out)>;

void tree_finish(Tree &t, int32_t status, double result) {
    t.finished = true;
    t.status = status;
    t.result = result;
}

// simplex() on the root has run (src/YALPS.ts:79): :89-107
void tree_begin(Tree &t, int32_t root_status, double root_result) {
    if (root_status != YALPS_OPTIMAL || t.nints == 0) return tree_finish(t, root_status, root_result);
    int32_t variable = 0;
    double value = 0.0, frac = 0.0;
    milp_most_fractional(t.best, t.w, t.ints, t.nints, &variable, &value, &frac);
    if (frac <= t.precision) return tree_finish(t, YALPS_OPTIMAL, root_result); // :94-95
    milp_push_first(t.branches, root_result, variable, value);
    t.threshold = root_result * (1.0 - t.sign * t.tolerance);
    t.stop_time = t.timeout + milp_now_ms();
    t.timedout = milp_now_ms() >= t.stop_time;
}

// :105-176, until the tree is finished or has popped a node whose result is not in its cache
void tree_advance(Tree &t, int32_t index, yalps_milpbatch_consumed_fn consumed, void *user) {
    while (!t.finished) {
        if (!t.has_pending) {
            if (!(t.iter < t.max_iter && !t.branches.empty() && t.best_eval >= t.threshold && !t.timedout)) break;
            t.pending = milp_pop(t.branches);
            if (t.pending.eval > t.best_eval) break; // :119
            t.has_pending = true;
        }
        auto it = t.cache.find(t.pending.cuts);
        if (it == t.cache.end()) return; // (the next round evaluates it)
        MilpEval ev = std::move(it->second);
        t.cache.erase(it);
        t.has_pending = false;
        const MilpBranch &br = t.pending;
        t.used++;
        if (consumed) {
            std::vector<int32_t> sg, vr;
            std::vector<double> vl;
            for (const MilpCut &cut : br.cuts) {
                sg.push_back(cut.sign);
                vr.push_back(cut.variable);
                vl.push_back(cut.value);
            }
            consumed(user, index, br.eval, (int32_t)sg.size(), sg.data(), vr.data(), vl.data());
        }
        if (ev.status == YALPS_OPTIMAL && ev.result < t.best_eval) {
            int32_t variable = 0;
            double value = 0.0, frac = 0.0;
            milp_most_fractional(ev.view, t.w, t.ints, t.nints, &variable, &value, &frac);
            if (frac <= t.precision) { // :131-136
                t.found = true;
                t.best_eval = ev.result;
                t.best = std::move(ev.view);
            } else { // :137-158
                milp_push_children(t.branches, br, variable, value, ev.result);
            }
        }
        t.timedout = milp_now_ms() >= t.stop_time;
        t.iter += 1.0;
    }
    if (t.finished) return;
    const bool unfinished = (t.timedout || t.iter >= t.max_iter) && !t.branches.empty() && t.best_eval >= t.threshold; // :166-173
    tree_finish(t, unfinished ? YALPS_MILPBATCH_TIMEDOUT : (t.found ? YALPS_OPTIMAL : YALPS_INFEASIBLE), t.found ? t.best_eval : NAN);
}

// Rounds until every tree has finished: the wanted nodes of all unfinished trees in one eval call, results into the
// caches, then every tree advances.
int lockstep(std::vector<Tree> &trees, int32_t node_batch, const EvalFn &eval, yalps_milpbatch_consumed_fn consumed, void *user,
             int64_t *rounds_out) {
    int64_t rounds = 0;
    for (size_t i = 0; i < trees.size(); i++) tree_advance(trees[i], (int32_t)i, consumed, user);
    std::vector<int32_t> model, sg, vr;
    std::vector<int64_t> off;
    std::vector<double> vl;
    std::vector<const MilpCuts *> which;
    std::vector<MilpEval> out;
    for (;;) {
        model.clear(), sg.clear(), vr.clear(), vl.clear(), which.clear();
        off.assign(1, 0);
        for (size_t i = 0; i < trees.size(); i++) {
            Tree &t = trees[i];
            if (t.finished) continue;
            for (const MilpCuts *cs : milp_wanted(t.branches, t.pending.cuts, node_batch, t.cache)) {
                for (const MilpCut &cut : *cs) {
                    sg.push_back(cut.sign);
                    vr.push_back(cut.variable);
                    vl.push_back(cut.value);
                }
                off.push_back((int64_t)sg.size());
                model.push_back((int32_t)i);
                which.push_back(cs);
            }
        }
        if (model.empty()) break;
        out.assign(model.size(), MilpEval());
        if (int rc = eval(model, off, sg, vr, vl, out)) return rc;
        rounds++;
        for (size_t k = 0; k < model.size(); k++) {
            Tree &t = trees[(size_t)model[k]];
            t.evaluated++;
            t.cache.emplace(*which[k], std::move(out[k]));
        }
        for (size_t i = 0; i < trees.size(); i++) tree_advance(trees[i], (int32_t)i, consumed, user);
    }
    if (rounds_out) *rounds_out = rounds;
    return 0;
}

int validate_models(int32_t count, const int32_t *width, const int32_t *height, const int64_t *ioff, const int32_t *ints,
                    int32_t node_batch) {
    if (count < 0) return fail(YALPS_E_ARG, "yalps_milpbatch: count < 0");
    if (node_batch < 1) return fail(YALPS_E_ARG, "yalps_milpbatch: node_batch must be at least 1");
    if (count == 0) return 0;
    if (!width || !height || !ioff) return fail(YALPS_E_ARG, "yalps_milpbatch: width / height / int_offsets is NULL");
    if (ioff[0] < 0) return fail(YALPS_E_ARG, "yalps_milpbatch: model 0: negative integer offset");
    for (int32_t i = 0; i < count; i++) {
        const std::string who = "yalps_milpbatch: model " + std::to_string(i) + ": ";
        const int64_t w = width[i], h = height[i];
        if (w < 1 || h < 1) return fail(YALPS_E_ARG, who + "width and height must be at least 1");
        if (ioff[i + 1] < ioff[i]) return fail(YALPS_E_ARG, who + "integer offsets decrease");
        const int64_t n = ioff[i + 1] - ioff[i];
        if (n > 0 && !ints) return fail(YALPS_E_ARG, who + "integers is NULL");
        if (8 * w * (h + 2 * n) > YALPS_MILPBATCH_MAX_BYTES)
            return fail(YALPS_E_ARG, who + "largest node of " + std::to_string(8 * w * (h + 2 * n)) + " bytes is above the batch limit of " +
                                         std::to_string((long long)YALPS_MILPBATCH_MAX_BYTES));
        for (int64_t k = ioff[i]; k < ioff[i + 1]; k++)
            if (ints[k] < 1 || ints[k] >= w) return fail(YALPS_E_ARG, who + "integer variable " + std::to_string(ints[k]) + " out of range");
    }
    return 0;
}

int validate_nodes(int32_t n_roots, const int32_t *rw, const int32_t *rh, int32_t count, const int32_t *root, const int64_t *off,
                   const int32_t *cvar) {
    if (count < 0 || n_roots < 0) return fail(YALPS_E_ARG, "yalps_milpbatch: count < 0");
    if (count == 0) return 0;
    if (!root || !off || !rw || !rh) return fail(YALPS_E_ARG, "yalps_milpbatch: root_index / cut_offsets is NULL");
    if (off[0] < 0) return fail(YALPS_E_ARG, "yalps_milpbatch: node 0: negative cut offset");
    for (int32_t k = 0; k < count; k++) {
        const std::string who = "yalps_milpbatch: node " + std::to_string(k) + ": ";
        if (root[k] < 0 || root[k] >= n_roots) return fail(YALPS_E_ARG, who + "root index " + std::to_string(root[k]) + " out of range");
        if (off[k + 1] < off[k]) return fail(YALPS_E_ARG, who + "cut offsets decrease");
        const int64_t w = rw[root[k]], h = rh[root[k]] + (off[k + 1] - off[k]);
        if (8 * w * h > YALPS_MILPBATCH_MAX_BYTES)
            return fail(YALPS_E_ARG, who + "tableau of " + std::to_string(8 * w * h) + " bytes is above the batch limit of " +
                                         std::to_string((long long)YALPS_MILPBATCH_MAX_BYTES));
        if (off[k + 1] > off[k] && !cvar) return fail(YALPS_E_ARG, who + "cut_var is NULL");
        for (int64_t c = off[k]; c < off[k + 1]; c++)
            if (cvar[c] < 1 || cvar[c] >= w) return fail(YALPS_E_ARG, who + "cut on variable " + std::to_string(cvar[c]) + " out of range");
    }
    return 0;
}
} // namespace

struct yalps_milpbatch {
    yalps_lpbatch *lp = nullptr; // the root pass: device, stream, events, the kept root tableaux
    std::vector<int32_t> root_check;
    QueueBufs q;
    DevBuf ndesc, csign, cvar, cval, height;
    // the last node pass
    std::vector<NodeDesc> nodes;
    std::vector<int32_t> h_height, h_pos, h_var;
    std::vector<double> h_result, h_col0;
    std::vector<long long> h_pivots;
    bool in_solve = false;
    // the last solve
    std::vector<Tree> trees;
    std::vector<int32_t> ints;
    // info
    std::string info, lines;
    std::vector<std::string> rerun_ids;
    int64_t rounds = 0, launches = 0;
    double gpu_ms = 0.0;
};

namespace {
void info_reset(yalps_milpbatch *b) {
    b->lines.clear();
    b->rerun_ids.clear();
    b->rounds = b->launches = 0;
    b->gpu_ms = 0.0;
}
void info_close(yalps_milpbatch *b) {
    std::string ids;
    for (const std::string &s : b->rerun_ids) ids += (ids.empty() ? "" : ",") + s;
    char head[160];
    std::snprintf(head, sizeof head, "rounds=%lld launches=%lld reruns=%zu gpu_us=%lld rerun_nodes=[", (long long)b->rounds,
                  (long long)b->launches, b->rerun_ids.size(), (long long)std::llround(b->gpu_ms * 1000.0));
    b->info = head + ids + "]\n" + b->lines;
}

// the root pass's launches, as the LP library's info spells them
void info_roots(yalps_milpbatch *b) {
    const std::string &t = b->lp->info;
    const size_t nl = t.find('\n');
    if (nl == std::string::npos) return;
    b->lines += t.substr(nl + 1);
    b->launches += std::count(t.begin() + (long)nl + 1, t.end(), '\n');
}

int roots_impl(yalps_milpbatch *b, int32_t count, const int32_t *width, const int32_t *height, const int64_t *off,
               const int32_t *row, const int32_t *col, const double *val, const double *precision, const double *maxPivots,
               const int32_t *checkCycles, int32_t *status_out, double *result_out, int64_t *pivots_out) {
    b->nodes.clear();
    b->root_check.clear();
    float ms = 0.f;
    if (int rc = lp_solve_impl(b->lp, count, width, height, off, row, col, val, precision, maxPivots, checkCycles, 1, status_out,
                            result_out, pivots_out, &ms)) {
        b->lp->descs.clear();
        return rc;
    }
    b->root_check.assign(checkCycles, checkCycles + count);
    b->gpu_ms += ms;
    info_roots(b);
    return 0;
}

// The node pass: descriptors and cuts up, the launches, the history reruns.  Leaves every node's outputs on the host.
int nodes_impl(yalps_milpbatch *b, int32_t count, const int32_t *root, const int64_t *off, const int32_t *csign, const int32_t *cvar,
               const double *cval, const double *max_pivots, int32_t keep) {
    yalps_lpbatch *lp = b->lp;
    const std::vector<LpDesc> &R = lp->descs;
    b->nodes.clear();
    {
        std::vector<int32_t> rw(R.size()), rh(R.size());
        for (size_t i = 0; i < R.size(); i++) rw[i] = R[i].w, rh[i] = R[i].h;
        if (int rc = validate_nodes((int32_t)R.size(), rw.data(), rh.data(), count, root, off, cvar)) return rc;
    }
    if (count > 0 && off[count] > off[0] && (!csign || !cval)) return fail(YALPS_E_ARG, "yalps_milpbatch_nodes: cut_sign / cut_val is NULL");
    b->q.keep = keep != 0;
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(lp->device));
    hipStream_t s = lp->stream;
    const size_t n = (size_t)count;
    std::vector<NodeDesc> &N = b->nodes;
    N.resize(n);
    long long col0_total = 0, perm_total = 0, tab_total = 0;
    const int64_t base = off[0];
    for (size_t k = 0; k < n; k++) {
        NodeDesc &d = N[k];
        const LpDesc &r = R[(size_t)root[k]];
        d.root = root[k];
        d.ncuts = (int32_t)(off[k + 1] - off[k]);
        d.cut_lo = off[k] - base;
        const int32_t h = r.h + d.ncuts;
        d.col0_off = col0_total;
        d.perm_off = perm_total;
        d.tab_off = tab_total;
        d.max_pivots = max_pivots ? max_pivots[k] : r.max_pivots;
        d.aux_hbm = lp_aux_hbm(r.w, h) ? 1 : 0;
        d.pad_ = 0;
        col0_total += (h + 1) & ~1; // (even offsets: 16-byte aligned column 0)
        perm_total += r.w + h;
        tab_total += (long long)r.w * h;
    }
    const size_t ncuts = (size_t)(off[count] - base);
    if (int rc = ensure(b->ndesc, sizeof(NodeDesc) * n)) return rc;
    if (int rc = ensure(b->csign, sizeof(int32_t) * ncuts)) return rc;
    if (int rc = ensure(b->cvar, sizeof(int32_t) * ncuts)) return rc;
    if (int rc = ensure(b->cval, sizeof(double) * ncuts)) return rc;
    if (int rc = ensure(b->height, sizeof(int32_t) * n)) return rc;
    if (int rc = ensure_outputs(b->q, n, (size_t)col0_total, (size_t)perm_total, (size_t)tab_total)) return rc;
    HIP_TRY(hipMemcpyAsync(b->ndesc.p, N.data(), sizeof(NodeDesc) * n, hipMemcpyHostToDevice, s));
    if (ncuts) {
        HIP_TRY(hipMemcpyAsync(b->csign.p, csign + base, sizeof(int32_t) * ncuts, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->cvar.p, cvar + base, sizeof(int32_t) * ncuts, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(b->cval.p, cval + base, sizeof(double) * ncuts, hipMemcpyHostToDevice, s));
    }
    if (int rc = reset_status(b->q, s, n)) return rc;
    b->h_height.assign(n, 0);
    b->h_result.assign(n, NAN);
    b->h_pivots.assign(n, 0);
    b->h_col0.resize((size_t)col0_total);
    b->h_pos.resize((size_t)perm_total);
    b->h_var.resize((size_t)perm_total);

    // every launch of a pass enqueued, then every output on its way back, one wait
    QueueRun run;
    const int rc = run_queue(
        *lp, b->q, kNodeKernels, QueueText{"yalps_milpbatch", false, "yalps_milpbatch_nodes", "node"}, n,
        [&](int32_t k, int *w, int *h) {
            const LpDesc &r = R[(size_t)N[k].root];
            return *w = r.w, *h = r.h + N[k].ncuts, b->root_check[(size_t)N[k].root] != 0;
        },
        [&](NodeLaunch &a) {
            a.roots = lp->desc.as<const LpDesc>();
            a.root_tab = lp->q.tab.as<const double>();
            a.root_pos = lp->q.pos.as<const int32_t>();
            a.root_var = lp->q.var.as<const int32_t>();
            a.node = b->ndesc.as<const NodeDesc>();
            a.cut_sign = b->csign.as<const int32_t>();
            a.cut_var = b->cvar.as<const int32_t>();
            a.cut_val = b->cval.as<const double>();
            a.height = b->height.as<int32_t>();
        },
        [&]() -> int {
            HIP_TRY(hipMemcpyAsync(b->h_height.data(), b->height.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(b->h_result.data(), b->q.result.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(b->h_pivots.data(), b->q.pivots.p, sizeof(long long) * n, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(b->h_col0.data(), b->q.col0.p, sizeof(double) * (size_t)col0_total, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(b->h_pos.data(), b->q.pos.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
            HIP_TRY(hipMemcpyAsync(b->h_var.data(), b->q.var.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
            return 0;
        },
        [&](const Launch &L, const std::string &kernel, int pass, int, long long hist_cap) {
            char line[256];
            std::snprintf(line, sizeof line, "launch=%lld round=%lld pass=%d kernel=%s class=%d nodes=%zu grid=%d lds=%zu hist_cap=%lld\n",
                          (long long)b->launches++, (long long)b->rounds, pass, kernel.c_str(), L.cls, L.items.size(), L.grid, L.shmem, hist_cap);
            if (b->lines.size() < ((size_t)1 << 20)) b->lines += line; // (a long solve: the text stops growing, the counts do not)
        },
        run);
    if (rc) return rc;
    b->gpu_ms += run.ms;
    for (int32_t k : run.reruns) b->rerun_ids.push_back((b->in_solve ? std::to_string(b->rounds) + ":" : "") + std::to_string(k)); // (a solve: round:node)
    return 0;
}

void eval_from_node(const yalps_milpbatch *b, size_t k, MilpEval &ev) {
    const NodeDesc &d = b->nodes[k];
    const int32_t w = b->lp->descs[(size_t)d.root].w, h = b->h_height[k];
    ev.status = b->q.h_status[k];
    ev.result = b->h_result[k];
    if (ev.status != YALPS_OPTIMAL) return;
    ev.view.height = h;
    ev.view.col0.assign(b->h_col0.begin() + d.col0_off, b->h_col0.begin() + d.col0_off + h);
    ev.view.pos.assign(b->h_pos.begin() + d.perm_off, b->h_pos.begin() + d.perm_off + w + h);
    ev.view.var.assign(b->h_var.begin() + d.perm_off, b->h_var.begin() + d.perm_off + w + h);
}

void trees_out(const std::vector<Tree> &trees, int32_t *status_out, double *result_out, int64_t *stats_out) {
    for (size_t i = 0; i < trees.size(); i++) {
        if (status_out) status_out[i] = trees[i].status;
        if (result_out) result_out[i] = trees[i].result;
        if (stats_out) stats_out[2 * i] = trees[i].used, stats_out[2 * i + 1] = trees[i].evaluated;
    }
}

int solve_milps(yalps_milpbatch *b, int32_t count, const int32_t *width, const int32_t *height, const int64_t *off, const int32_t *row,
                const int32_t *col, const double *val, const int64_t *ioff, const int32_t *ints, const double *sign,
                const double *precision, const double *maxPivots, const int32_t *checkCycles, const double *tolerance,
                const double *timeout, const double *maxIter, int32_t node_batch, int32_t *status_out, double *result_out,
                int64_t *stats_out, int64_t *call_stats) {
    b->trees.clear();
    if (int rc = validate_models(count, width, height, ioff, ints, node_batch)) return rc;
    if (count > 0 && (!sign || !precision || !maxPivots || !checkCycles || !tolerance || !timeout || !maxIter))
        return fail(YALPS_E_ARG, "yalps_milpbatch_solve: an option array is NULL");
    std::vector<int32_t> rstatus((size_t)count);
    std::vector<double> rresult((size_t)count);
    if (int rc = roots_impl(b, count, width, height, off, row, col, val, precision, maxPivots, checkCycles, rstatus.data(),
                            rresult.data(), nullptr))
        return rc;
    if (count > 0) b->ints.assign(ints + ioff[0], ints + ioff[count]);
    std::vector<Tree> trees((size_t)count);
    for (int32_t i = 0; i < count; i++) {
        Tree &t = trees[(size_t)i];
        const LpDesc &d = b->lp->descs[(size_t)i];
        t.w = d.w, t.h = d.h;
        t.nints = (int32_t)(ioff[i + 1] - ioff[i]);
        t.ints = b->ints.data() + (ioff[i] - ioff[0]);
        t.sign = sign[i], t.precision = precision[i], t.tolerance = tolerance[i], t.timeout = timeout[i], t.max_iter = maxIter[i];
        t.best.height = d.h;
        t.best.col0.assign(b->lp->h_col0.begin() + d.col0_off, b->lp->h_col0.begin() + d.col0_off + d.h);
        t.best.pos.assign(b->lp->h_pos.begin() + d.perm_off, b->lp->h_pos.begin() + d.perm_off + d.w + d.h);
        t.best.var.assign(b->lp->h_var.begin() + d.perm_off, b->lp->h_var.begin() + d.perm_off + d.w + d.h);
        tree_begin(t, rstatus[(size_t)i], rresult[(size_t)i]);
    }
    b->in_solve = true;
    const EvalFn eval = [&](const std::vector<int32_t> &model, const std::vector<int64_t> &coff, const std::vector<int32_t> &sg,
                            const std::vector<int32_t> &vr, const std::vector<double> &vl, std::vector<MilpEval> &out) -> int {
        if (int rc = nodes_impl(b, (int32_t)model.size(), model.data(), coff.data(), sg.data(), vr.data(), vl.data(), nullptr, 0)) return rc;
        for (size_t k = 0; k < model.size(); k++) eval_from_node(b, k, out[k]);
        b->rounds++;
        return 0;
    };
    const int rc = lockstep(trees, node_batch, eval, nullptr, nullptr, nullptr);
    b->in_solve = false;
    if (rc) return rc;
    b->trees = std::move(trees);
    trees_out(b->trees, status_out, result_out, stats_out);
    if (call_stats) {
        call_stats[0] = b->rounds;
        call_stats[1] = b->launches;
        call_stats[2] = (int64_t)std::llround(b->gpu_ms * 1000.0);
    }
    return 0;
}
} // namespace

extern "C" {

const char *yalps_milpbatch_last_error(void) { return g_err.c_str(); }

int32_t yalps_milpbatch_create(int32_t device, void *hip_stream, yalps_milpbatch **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_milpbatch_create: out is NULL");
    *out = nullptr;
    yalps_lpbatch *lp = nullptr;
    if (int rc = lp_create(device, hip_stream, &lp)) return rc;
    for (const KernelForm<NodeLaunch> &f : kNodeKernels.forms) {
        const hipError_t e = hipFuncSetAttribute(reinterpret_cast<const void *>(f.fn), hipFuncAttributeMaxDynamicSharedMemorySize,
                                                 (int)SMALL_LDS_MAX);
        if (e != hipSuccess) {
            lp_destroy(lp);
            return fail(YALPS_E_DEVICE, std::string("hipFuncSetAttribute: ") + hipGetErrorString(e));
        }
    }
    yalps_milpbatch *b = new yalps_milpbatch();
    b->lp = lp;
    b->q.hist_first = std::max(1, env_int("YALPS_MILPBATCH_HIST", (int)HIST_FIRST)); // (test hook: forces the node rerun)
    b->info = "rounds=0 launches=0 reruns=0 gpu_us=0 rerun_nodes=[]\n";
    *out = b;
    return 0;
}

void yalps_milpbatch_destroy(yalps_milpbatch *b) {
    if (!b) return;
    (void)hipSetDevice(b->lp->device);
    if (b->lp->stream) (void)hipStreamSynchronize(b->lp->stream);
    release(b->q);
    release({&b->ndesc, &b->csign, &b->cvar, &b->cval, &b->height});
    lp_destroy(b->lp);
    delete b;
}

int32_t yalps_milpbatch_roots(yalps_milpbatch *b, int32_t count, const int32_t *width, const int32_t *height,
                              const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                              const double *precision, const double *maxPivots, const int32_t *checkCycles,
                              int32_t *status_out, double *result_out, int64_t *pivots_out) {
    if (!b) return fail(YALPS_E_ARG, "yalps_milpbatch_roots: handle is NULL");
    b->trees.clear();
    info_reset(b);
    const int rc = roots_impl(b, count, width, height, cell_offsets, row, col, val, precision, maxPivots, checkCycles, status_out,
                              result_out, pivots_out);
    info_close(b);
    return rc;
}

int32_t yalps_milpbatch_root(yalps_milpbatch *b, int32_t i, double *col0, int32_t *positionOfVariable,
                             int32_t *variableAtPosition, double *matrix) {
    if (!b || i < 0 || (size_t)i >= b->lp->descs.size()) return fail(YALPS_E_ARG, "yalps_milpbatch_root: no such root in the last root pass");
    const LpDesc &d = b->lp->descs[(size_t)i];
    const size_t np = (size_t)d.w + (size_t)d.h;
    if (col0) std::memcpy(col0, b->lp->h_col0.data() + d.col0_off, sizeof(double) * (size_t)d.h);
    if (positionOfVariable) std::memcpy(positionOfVariable, b->lp->h_pos.data() + d.perm_off, sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, b->lp->h_var.data() + d.perm_off, sizeof(int32_t) * np);
    if (matrix) {
        HIP_TRY(hipSetDevice(b->lp->device));
        HIP_TRY(hipMemcpyAsync(matrix, b->lp->q.tab.as<const double>() + d.tab_off, sizeof(double) * (size_t)d.w * (size_t)d.h,
                               hipMemcpyDeviceToHost, b->lp->stream));
        HIP_TRY(hipStreamSynchronize(b->lp->stream));
    }
    return 0;
}

int32_t yalps_milpbatch_validate_nodes(int32_t n_roots, const int32_t *root_width, const int32_t *root_height, int32_t count,
                                       const int32_t *root_index, const int64_t *cut_offsets, const int32_t *cut_var) {
    return validate_nodes(n_roots, root_width, root_height, count, root_index, cut_offsets, cut_var);
}

int32_t yalps_milpbatch_nodes(yalps_milpbatch *b, int32_t count, const int32_t *root_index, const int64_t *cut_offsets,
                              const int32_t *cut_sign, const int32_t *cut_var, const double *cut_val,
                              const double *maxPivots_override, int32_t keep_tableaux, int32_t *status_out,
                              double *result_out, int64_t *pivots_out, int32_t *height_out) {
    if (!b) return fail(YALPS_E_ARG, "yalps_milpbatch_nodes: handle is NULL");
    b->trees.clear();
    info_reset(b);
    const int rc = nodes_impl(b, count, root_index, cut_offsets, cut_sign, cut_var, cut_val, maxPivots_override, keep_tableaux);
    info_close(b);
    if (rc) {
        b->nodes.clear();
        return rc;
    }
    const size_t n = (size_t)count;
    if (status_out) std::memcpy(status_out, b->q.h_status.data(), sizeof(int32_t) * n);
    if (height_out) std::memcpy(height_out, b->h_height.data(), sizeof(int32_t) * n);
    if (result_out) std::memcpy(result_out, b->h_result.data(), sizeof(double) * n);
    if (pivots_out)
        for (size_t k = 0; k < n; k++) pivots_out[k] = b->h_pivots[k];
    return 0;
}

int32_t yalps_milpbatch_node(yalps_milpbatch *b, int32_t k, double *col0, int32_t *positionOfVariable,
                             int32_t *variableAtPosition) {
    if (!b || k < 0 || (size_t)k >= b->nodes.size()) return fail(YALPS_E_ARG, "yalps_milpbatch_node: no such node in the last node pass");
    const NodeDesc &d = b->nodes[(size_t)k];
    const size_t h = (size_t)b->h_height[(size_t)k], np = (size_t)b->lp->descs[(size_t)d.root].w + h;
    if (col0) std::memcpy(col0, b->h_col0.data() + d.col0_off, sizeof(double) * h);
    if (positionOfVariable) std::memcpy(positionOfVariable, b->h_pos.data() + d.perm_off, sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, b->h_var.data() + d.perm_off, sizeof(int32_t) * np);
    return 0;
}

int32_t yalps_milpbatch_node_tableau(yalps_milpbatch *b, int32_t k, double *matrix) {
    if (!b || k < 0 || (size_t)k >= b->nodes.size() || !matrix)
        return fail(YALPS_E_ARG, "yalps_milpbatch_node_tableau: no such node in the last node pass");
    if (!b->q.keep) return fail(YALPS_E_ARG, "yalps_milpbatch_node_tableau: the last node pass did not keep its tableaux (keep_tableaux)");
    const NodeDesc &d = b->nodes[(size_t)k];
    const size_t w = (size_t)b->lp->descs[(size_t)d.root].w, h = (size_t)b->h_height[(size_t)k];
    HIP_TRY(hipSetDevice(b->lp->device));
    HIP_TRY(hipMemcpyAsync(matrix, b->q.tab.as<const double>() + d.tab_off, sizeof(double) * w * h, hipMemcpyDeviceToHost,
                           b->lp->stream));
    HIP_TRY(hipStreamSynchronize(b->lp->stream));
    return 0;
}

int32_t yalps_milpbatch_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *int_offsets,
                                 const int32_t *integers, int32_t node_batch) {
    return validate_models(count, width, height, int_offsets, integers, node_batch);
}

int32_t yalps_milpbatch_solve(yalps_milpbatch *b, int32_t count, const int32_t *width, const int32_t *height,
                              const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                              const int64_t *int_offsets, const int32_t *integers, const double *sign,
                              const double *precision, const double *maxPivots, const int32_t *checkCycles,
                              const double *tolerance, const double *timeout_ms, const double *maxIterations,
                              int32_t node_batch, int32_t *status_out, double *result_out, int64_t *stats_out,
                              int64_t *call_stats_out) {
    if (!b) return fail(YALPS_E_ARG, "yalps_milpbatch_solve: handle is NULL");
    info_reset(b);
    const int rc = solve_milps(b, count, width, height, cell_offsets, row, col, val, int_offsets, integers, sign, precision, maxPivots,
                               checkCycles, tolerance, timeout_ms, maxIterations, node_batch, status_out, result_out, stats_out,
                               call_stats_out);
    info_close(b);
    b->nodes.clear(); // (the node pass of the last round is the driver's, not the caller's)
    return rc;
}

int32_t yalps_milpbatch_solution(yalps_milpbatch *b, int32_t i, int32_t *height_out, double *col0, int32_t *positionOfVariable,
                                 int32_t *variableAtPosition) {
    if (!b || i < 0 || (size_t)i >= b->trees.size()) return fail(YALPS_E_ARG, "yalps_milpbatch_solution: no such model in the last solve");
    const Tree &t = b->trees[(size_t)i];
    const size_t h = (size_t)t.best.height, np = (size_t)t.w + h;
    if (height_out) *height_out = t.best.height;
    if (col0) std::memcpy(col0, t.best.col0.data(), sizeof(double) * h);
    if (positionOfVariable) std::memcpy(positionOfVariable, t.best.pos.data(), sizeof(int32_t) * np);
    if (variableAtPosition) std::memcpy(variableAtPosition, t.best.var.data(), sizeof(int32_t) * np);
    return 0;
}

int32_t yalps_milpbatch_search(int32_t count, const int32_t *width, const int32_t *height, const int32_t *root_status,
                               const double *root_result, const double *root_col0, const int32_t *root_pos,
                               const int32_t *root_var, const int64_t *int_offsets, const int32_t *integers,
                               const double *sign, const double *precision, const double *tolerance,
                               const double *timeout_ms, const double *maxIterations, int32_t node_batch,
                               yalps_milpbatch_eval_fn eval, yalps_milpbatch_consumed_fn consumed, void *user,
                               int32_t *status_out, double *result_out, int32_t *height_out, double *col0_out,
                               int32_t *pos_out, int32_t *var_out, int64_t *stats_out, int64_t *rounds_out) {
    if (int rc = validate_models(count, width, height, int_offsets, integers, node_batch)) return rc;
    if (!eval) return fail(YALPS_E_ARG, "yalps_milpbatch_search: eval is NULL");
    if (count > 0 && (!root_status || !root_result || !root_col0 || !root_pos || !root_var || !sign || !precision || !tolerance ||
                      !timeout_ms || !maxIterations || !height_out || !col0_out || !pos_out || !var_out))
        return fail(YALPS_E_ARG, "yalps_milpbatch_search: an argument is NULL");
    std::vector<Tree> trees((size_t)count);
    size_t c0 = 0, p0 = 0;
    for (int32_t i = 0; i < count; i++) {
        Tree &t = trees[(size_t)i];
        t.w = width[i], t.h = height[i];
        t.nints = (int32_t)(int_offsets[i + 1] - int_offsets[i]);
        t.ints = integers + int_offsets[i];
        t.sign = sign[i], t.precision = precision[i], t.tolerance = tolerance[i], t.timeout = timeout_ms[i], t.max_iter = maxIterations[i];
        t.best.height = t.h;
        t.best.col0.assign(root_col0 + c0, root_col0 + c0 + t.h);
        t.best.pos.assign(root_pos + p0, root_pos + p0 + t.w + t.h);
        t.best.var.assign(root_var + p0, root_var + p0 + t.w + t.h);
        c0 += (size_t)t.h;
        p0 += (size_t)t.w + (size_t)t.h;
        tree_begin(t, root_status[i], root_result[i]);
    }
    std::vector<int32_t> st, hg, ps, vs;
    std::vector<double> rs, cs;
    const EvalFn call = [&](const std::vector<int32_t> &model, const std::vector<int64_t> &coff, const std::vector<int32_t> &sg,
                            const std::vector<int32_t> &vr, const std::vector<double> &vl, std::vector<MilpEval> &out) -> int {
        const size_t n = model.size();
        size_t rows = 0, perms = 0;
        for (size_t k = 0; k < n; k++) {
            const Tree &t = trees[(size_t)model[k]];
            const size_t h = (size_t)t.h + (size_t)(coff[k + 1] - coff[k]);
            rows += h;
            perms += (size_t)t.w + h;
        }
        st.assign(n, YALPS_CYCLED), hg.assign(n, 0), rs.assign(n, NAN);
        cs.assign(rows, 0.0), ps.assign(perms, 0), vs.assign(perms, 0);
        const int32_t rc = eval(user, (int32_t)n, model.data(), coff.data(), sg.data(), vr.data(), vl.data(), st.data(), rs.data(),
                                hg.data(), cs.data(), ps.data(), vs.data());
        if (rc < 0) return fail(rc, "yalps_milpbatch_search: the evaluator failed");
        size_t c = 0, p = 0;
        for (size_t k = 0; k < n; k++) {
            const Tree &t = trees[(size_t)model[k]];
            const size_t h = (size_t)t.h + (size_t)(coff[k + 1] - coff[k]), np = (size_t)t.w + h;
            out[k].status = st[k];
            out[k].result = rs[k];
            if (st[k] == YALPS_OPTIMAL) {
                if ((size_t)hg[k] != h) return fail(YALPS_E_ARG, "yalps_milpbatch_search: the evaluator returned a node of another height");
                out[k].view.height = (int32_t)h;
                out[k].view.col0.assign(cs.begin() + (long)c, cs.begin() + (long)(c + h));
                out[k].view.pos.assign(ps.begin() + (long)p, ps.begin() + (long)(p + np));
                out[k].view.var.assign(vs.begin() + (long)p, vs.begin() + (long)(p + np));
            }
            c += h;
            p += np;
        }
        return 0;
    };
    if (int rc = lockstep(trees, node_batch, call, consumed, user, rounds_out)) return rc;
    trees_out(trees, status_out, result_out, stats_out);
    c0 = p0 = 0;
    for (int32_t i = 0; i < count; i++) {
        const Tree &t = trees[(size_t)i];
        const size_t h = (size_t)t.best.height;
        height_out[i] = t.best.height;
        std::memcpy(col0_out + c0, t.best.col0.data(), sizeof(double) * h);
        std::memcpy(pos_out + p0, t.best.pos.data(), sizeof(int32_t) * ((size_t)t.w + h));
        std::memcpy(var_out + p0, t.best.var.data(), sizeof(int32_t) * ((size_t)t.w + h));
        c0 += (size_t)t.h + 2 * (size_t)t.nints;
        p0 += (size_t)t.w + (size_t)t.h + 2 * (size_t)t.nints;
    }
    return 0;
}

int32_t yalps_milpbatch_info(const yalps_milpbatch *b, char *buf, int32_t len) {
    if (!b || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_milpbatch_info: bad argument");
    return info_out(b->info, buf, len);
}

} // extern "C"
