// milp_tree.hip -- libyalps_milptree.so: a batch of independent MILPs, every branch-and-cut tree walked on the device
// (include/yalps_milptree.h).  The root pass is libyalps_lpbatch.so's host code and kernels (lp_batch_host.inc,
// lp_batch_kernel.cuh) with kept tableaux, compiled again here as milp_batch.hip and lp_warm.hip do; the tree pass is
// milp_tree_kernel on the launches plan_launches (wg_queue_host.inc) makes; the search rules are milp_tree_rules.cuh, which
// yalps_milptree_search runs on the host.
// A library of its own: nothing here is linked into libyalps_hip.so, libyalps_lpbatch.so or libyalps_milpbatch.so.
#include <hip/hip_runtime.h>

#include <algorithm>
#include <climits>
#include <cmath>
#include <cstdint>
#include <cstdio>
#include <cstdlib>
#include <cstring>
#include <string>
#include <vector>

#include "../../include/yalps_lpbatch.h"
#include "../../include/yalps_milptree.h"

#pragma clang fp contract(off)

#include "milp_tree_rules.cuh"

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_batch_kernel.cuh"
#include "milp_tree_kernel.cuh"
#include "wg_queue_host.inc"
#include "lp_batch_host.inc"

static_assert(YALPS_MILPTREE_MAX_BYTES == QUEUE_MAX_BYTES, "include/yalps_milptree.h");
#include "milp_tree_host.inc"
static_assert(TREE_TIMEDOUT == YALPS_MILPTREE_TIMEDOUT && TREE_OVERFLOW == YALPS_MILPTREE_OVERFLOW, "include/yalps_milptree.h");
} // namespace

#include "lp_batch_lib.inc"

struct yalps_milptree : TreePass {
    yalps_lpbatch *lp = nullptr; // the root pass: device, stream, events, the kept root tableaux
    // the last solve
    std::vector<int32_t> status, best_h, h_pos, h_var;
    std::vector<double> result, h_col0, h_trace;
    std::vector<long long> used, pivots;
    std::string info;
};

namespace {
int validate_models(int32_t count, const int32_t *width, const int32_t *height, const int64_t *ioff, const int32_t *ints,
                    const double *timeout) {
    if (count < 0) return fail(YALPS_E_ARG, "yalps_milptree: count < 0");
    if (count == 0) return 0;
    if (!width || !height || !ioff) return fail(YALPS_E_ARG, "yalps_milptree: width / height / int_offsets is NULL");
    if (ioff[0] < 0) return fail(YALPS_E_ARG, "yalps_milptree: model 0: negative integer offset");
    for (int32_t i = 0; i < count; i++) {
        const std::string who = "yalps_milptree: model " + std::to_string(i) + ": ";
        const int64_t w = width[i], h = height[i];
        if (w < 1 || h < 1) return fail(YALPS_E_ARG, who + "width and height must be at least 1");
        if (ioff[i + 1] < ioff[i]) return fail(YALPS_E_ARG, who + "integer offsets decrease");
        const int64_t n = ioff[i + 1] - ioff[i];
        if (n > 0 && !ints) return fail(YALPS_E_ARG, who + "integers is NULL");
        if (8 * w * (h + 2 * n) > YALPS_MILPTREE_MAX_BYTES)
            return fail(YALPS_E_ARG, who + "largest node of " + std::to_string(8 * w * (h + 2 * n)) + " bytes is above the batch limit of " +
                                         std::to_string((long long)YALPS_MILPTREE_MAX_BYTES));
        for (int64_t k = ioff[i]; k < ioff[i + 1]; k++)
            if (ints[k] < 1 || ints[k] >= w) return fail(YALPS_E_ARG, who + "integer variable " + std::to_string(ints[k]) + " out of range");
        if (timeout && !(timeout[i] == INFINITY || timeout[i] <= 0))
            return fail(YALPS_E_ARG, who + "timeout must be +Infinity or <= 0 (the device reads no clock)");
    }
    return 0;
}

void info_close(yalps_milptree *b) {
    char head[160];
    std::snprintf(head, sizeof head, "launches=%lld reruns=%zu overflows=%lld gpu_us=%lld rerun_trees=[", (long long)b->launches,
                  b->rerun_ids.size(), (long long)b->overflows, (long long)std::llround(b->gpu_ms * 1000.0));
    b->info = head + join_ids(b->rerun_ids) + "]\n" + b->lines;
}

int solve_trees(yalps_milptree *b, int32_t count, const int32_t *width, const int32_t *height, const int64_t *off, const int32_t *row,
                const int32_t *col, const double *val, const int64_t *ioff, const int32_t *ints, const double *sign,
                const double *precision, const double *maxPivots, const int32_t *checkCycles, const double *tolerance,
                const double *timeout, const double *maxIter, int32_t trace_cap, int32_t *status_out, double *result_out,
                int64_t *stats_out, int64_t *call_stats) {
    b->trees.clear();
    if (trace_cap < 0) return fail(YALPS_E_ARG, "yalps_milptree_solve: trace_cap < 0");
    if (count > 0 && (!sign || !precision || !maxPivots || !checkCycles || !tolerance || !timeout || !maxIter))
        return fail(YALPS_E_ARG, "yalps_milptree_solve: an option array is NULL");
    if (int rc = validate_models(count, width, height, ioff, ints, timeout)) return rc;
    float ms = 0.f;
    if (int rc = lp_solve_impl(b->lp, count, width, height, off, row, col, val, precision, maxPivots, checkCycles, 1, nullptr, nullptr,
                               nullptr, &ms)) {
        b->lp->descs.clear();
        return rc;
    }
    b->gpu_ms += ms;
    {
        const std::string &t = b->lp->info; // the root pass's launches, as the LP library's info spells them
        const size_t nl = t.find('\n');
        if (nl != std::string::npos) {
            b->lines += t.substr(nl + 1);
            b->launches += std::count(t.begin() + (long)nl + 1, t.end(), '\n');
        }
    }
    const size_t n = (size_t)count;
    if (call_stats) call_stats[0] = 0, call_stats[1] = b->launches, call_stats[2] = (int64_t)std::llround(b->gpu_ms * 1000.0);
    if (n == 0) return 0;
    HIP_TRY(hipSetDevice(b->lp->device));
    hipStream_t s = b->lp->stream;
    std::vector<TreeDesc> D(n);
    long long col0_total = 0, perm_total = 0, trace_total = 0;
    for (size_t i = 0; i < n; i++) {
        TreeDesc &d = D[i];
        const LpDesc &r = b->lp->descs[i];
        d.nints = (int32_t)(ioff[i + 1] - ioff[i]);
        d.maxcuts = std::max(1, 2 * d.nints);
        d.ints_off = ioff[i] - ioff[0];
        d.sign = sign[i], d.tolerance = tolerance[i], d.max_iter = maxIter[i];
        d.timedout = timeout[i] <= 0 ? 1 : 0;
        const int32_t hmax = r.h + 2 * d.nints;
        d.cls = lp_class(r.w, hmax);
        d.col0_off = col0_total, d.perm_off = perm_total, d.trace_off = trace_total;
        d.aux_hbm = lp_aux_hbm(r.w, hmax) ? 1 : 0;
        d.pad_ = 0;
        col0_total += (hmax + 1) & ~1;
        perm_total += r.w + hmax;
        trace_total += (long long)trace_cap * (4 + 2 * (long long)d.maxcuts);
    }
    const size_t nints = (size_t)(ioff[count] - ioff[0]);
    b->q.keep = false;
    b->trace_cap = trace_cap;
    if (int rc = ensure(b->tdesc, sizeof(TreeDesc) * n)) return rc;
    if (int rc = ensure(b->ints, sizeof(int32_t) * nints)) return rc;
    if (int rc = ensure(b->d_used, sizeof(long long) * n)) return rc;
    if (int rc = ensure(b->d_best_h, sizeof(int32_t) * n)) return rc;
    if (int rc = ensure(b->d_trace, sizeof(double) * (size_t)trace_total)) return rc;
    if (int rc = ensure_outputs(b->q, n, (size_t)col0_total, (size_t)perm_total, 0)) return rc;
    HIP_TRY(hipMemcpyAsync(b->tdesc.p, D.data(), sizeof(TreeDesc) * n, hipMemcpyHostToDevice, s));
    if (nints) HIP_TRY(hipMemcpyAsync(b->ints.p, ints + ioff[0], sizeof(int32_t) * nints, hipMemcpyHostToDevice, s));
    if (int rc = reset_status(b->q, s, n)) return rc;
    HIP_TRY(hipStreamSynchronize(s)); // (D is on this frame until it moves into the handle)
    b->trees = std::move(D);
    const TreeRoots roots{b->lp, b->lp->descs.data(), b->lp->desc.as<const LpDesc>(), &b->lp->q};
    if (int rc = trees_impl(b, roots, n, [&](int32_t i) { return checkCycles[i] != 0; }, "yalps_milptree")) return rc;

    b->status = b->q.h_status;
    b->result.assign(n, NAN);
    b->used.assign(n, 0);
    b->pivots.assign(n, 0);
    b->best_h.assign(n, 0);
    b->h_col0.resize((size_t)col0_total);
    b->h_pos.resize((size_t)perm_total);
    b->h_var.resize((size_t)perm_total);
    b->h_trace.resize((size_t)trace_total);
    HIP_TRY(hipMemcpyAsync(b->result.data(), b->q.result.p, sizeof(double) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->used.data(), b->d_used.p, sizeof(long long) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->pivots.data(), b->q.pivots.p, sizeof(long long) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->best_h.data(), b->d_best_h.p, sizeof(int32_t) * n, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_col0.data(), b->q.col0.p, sizeof(double) * (size_t)col0_total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_pos.data(), b->q.pos.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(b->h_var.data(), b->q.var.p, sizeof(int32_t) * (size_t)perm_total, hipMemcpyDeviceToHost, s));
    if (trace_total) HIP_TRY(hipMemcpyAsync(b->h_trace.data(), b->d_trace.p, sizeof(double) * (size_t)trace_total, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    for (size_t i = 0; i < n; i++) {
        if (b->status[i] == YALPS_MILPTREE_OVERFLOW) b->result[i] = NAN, b->best_h[i] = 0;
        if (status_out) status_out[i] = b->status[i];
        if (result_out) result_out[i] = b->result[i];
        if (stats_out) stats_out[2 * i] = b->used[i], stats_out[2 * i + 1] = b->pivots[i];
    }
    if (call_stats)
        call_stats[0] = (int64_t)b->rerun_ids.size(), call_stats[1] = b->launches, call_stats[2] = (int64_t)std::llround(b->gpu_ms * 1000.0);
    return 0;
}
} // namespace

extern "C" {

const char *yalps_milptree_last_error(void) { return g_err.c_str(); }

int32_t yalps_milptree_create(int32_t device, void *hip_stream, yalps_milptree **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_milptree_create: out is NULL");
    *out = nullptr;
    yalps_lpbatch *lp = nullptr;
    if (int rc = lp_create(device, hip_stream, &lp)) return rc;
    if (int rc = raise_lds_limit(kTreeKernels)) {
        const std::string why = g_err;
        lp_destroy(lp);
        g_err = why;
        return rc;
    }
    yalps_milptree *b = new yalps_milptree();
    b->lp = lp;
    b->q.hist_first = std::max(1, env_int("YALPS_MILPTREE_HIST", (int)HIST_FIRST)); // (test hooks: they force the reruns)
    b->arena_first = std::max(2, env_int("YALPS_MILPTREE_ARENA", ARENA_FIRST));
    b->arena_max = std::max(2, env_int("YALPS_MILPTREE_ARENA_MAX", ARENA_MAX));
    b->grid = std::max(0, env_int("YALPS_MILPTREE_GRID", 0));
    if (const int bytes = env_int("YALPS_MILPTREE_ARENA_BYTES", 0); bytes > 0) b->arena_bytes = bytes;
    b->info = "launches=0 reruns=0 overflows=0 gpu_us=0 rerun_trees=[]\n";
    *out = b;
    return 0;
}

void yalps_milptree_destroy(yalps_milptree *b) {
    if (!b) return;
    (void)hipSetDevice(b->lp->device);
    if (b->lp->stream) (void)hipStreamSynchronize(b->lp->stream);
    release(*b);
    lp_destroy(b->lp);
    delete b;
}

int32_t yalps_milptree_validate(int32_t count, const int32_t *width, const int32_t *height, const int64_t *int_offsets,
                                const int32_t *integers, const double *timeout_ms) {
    return validate_models(count, width, height, int_offsets, integers, timeout_ms);
}

int32_t yalps_milptree_solve(yalps_milptree *b, int32_t count, const int32_t *width, const int32_t *height,
                             const int64_t *cell_offsets, const int32_t *row, const int32_t *col, const double *val,
                             const int64_t *int_offsets, const int32_t *integers, const double *sign, const double *precision,
                             const double *maxPivots, const int32_t *checkCycles, const double *tolerance, const double *timeout_ms,
                             const double *maxIterations, int32_t trace_cap, int32_t *status_out, double *result_out,
                             int64_t *stats_out, int64_t *call_stats_out) {
    if (!b) return fail(YALPS_E_ARG, "yalps_milptree_solve: handle is NULL");
    b->lines.clear();
    b->rerun_ids.clear();
    b->launches = b->overflows = 0;
    b->gpu_ms = 0.0;
    const int rc = solve_trees(b, count, width, height, cell_offsets, row, col, val, int_offsets, integers, sign, precision, maxPivots,
                               checkCycles, tolerance, timeout_ms, maxIterations, trace_cap, status_out, result_out, stats_out,
                               call_stats_out);
    if (rc) b->trees.clear(); // (no last solve to read from)
    info_close(b);
    return rc;
}

int32_t yalps_milptree_solution(yalps_milptree *b, int32_t i, int32_t *height_out, double *col0, int32_t *positionOfVariable,
                                int32_t *variableAtPosition) {
    if (!b || i < 0 || (size_t)i >= b->trees.size()) return fail(YALPS_E_ARG, "yalps_milptree_solution: no such model in the last solve");
    const TreeDesc &d = b->trees[(size_t)i];
    const LpDesc &r = b->lp->descs[(size_t)i];
    const bool root = b->best_h[(size_t)i] == 0; // no incumbent: bestTableau is the root's (src/branchAndCut.ts:119)
    const size_t h = root ? (size_t)r.h : (size_t)b->best_h[(size_t)i], np = (size_t)r.w + h;
    if (height_out) *height_out = (int32_t)h;
    if (col0) std::memcpy(col0, root ? b->lp->h_col0.data() + r.col0_off : b->h_col0.data() + d.col0_off, sizeof(double) * h);
    if (positionOfVariable)
        std::memcpy(positionOfVariable, root ? b->lp->h_pos.data() + r.perm_off : b->h_pos.data() + d.perm_off, sizeof(int32_t) * np);
    if (variableAtPosition)
        std::memcpy(variableAtPosition, root ? b->lp->h_var.data() + r.perm_off : b->h_var.data() + d.perm_off, sizeof(int32_t) * np);
    return 0;
}

int32_t yalps_milptree_trace(yalps_milptree *b, int32_t i, int32_t *count_out, double *eval, int32_t *status, double *result,
                             int64_t *pivots, int32_t *height, int32_t *cut_sign, int32_t *cut_var, double *cut_val) {
    if (!b || i < 0 || (size_t)i >= b->trees.size()) return fail(YALPS_E_ARG, "yalps_milptree_trace: no such model in the last solve");
    const TreeDesc &d = b->trees[(size_t)i];
    const int32_t h0 = b->lp->descs[(size_t)i].h;
    const bool gone = b->status[(size_t)i] == YALPS_MILPTREE_OVERFLOW;
    const int32_t cnt = gone ? 0 : (int32_t)std::min<long long>(b->used[(size_t)i], b->trace_cap);
    if (count_out) *count_out = cnt;
    tree_trace_out(b->h_trace.data() + d.trace_off, d.maxcuts, cnt, h0, eval, status, result, pivots, height, cut_sign, cut_var, cut_val);
    return 0;
}

int32_t yalps_milptree_search(int32_t count, const int32_t *width, const int32_t *height, const int32_t *root_status,
                              const double *root_result, const double *root_col0, const int32_t *root_pos, const int32_t *root_var,
                              const int64_t *int_offsets, const int32_t *integers, const double *sign, const double *precision,
                              const double *tolerance, const double *timeout_ms, const double *maxIterations, int32_t arena,
                              int32_t arena_max, yalps_milptree_eval_fn eval, yalps_milptree_consumed_fn consumed, void *user,
                              int32_t *status_out, double *result_out, int32_t *height_out, double *col0_out, int32_t *pos_out,
                              int32_t *var_out, int64_t *stats_out, int64_t *reruns_out) {
    if (int rc = validate_models(count, width, height, int_offsets, integers, timeout_ms)) return rc;
    if (!eval) return fail(YALPS_E_ARG, "yalps_milptree_search: eval is NULL");
    if (arena < 2 || arena_max < arena) return fail(YALPS_E_ARG, "yalps_milptree_search: arena must be at least 2 and arena_max at least arena");
    if (count > 0 && (!root_status || !root_result || !root_col0 || !root_pos || !root_var || !sign || !precision || !tolerance ||
                      !timeout_ms || !maxIterations || !height_out || !col0_out || !pos_out || !var_out))
        return fail(YALPS_E_ARG, "yalps_milptree_search: an argument is NULL");
    size_t c0 = 0, p0 = 0, oc0 = 0, op0 = 0;
    int64_t reruns = 0;
    std::vector<double> mem, ncol0, seq_val, seq_eval;
    std::vector<int32_t> npos, nvar, sg, vr, seq_sg, seq_vr, seq_n;
    std::vector<double> vl;
    for (int32_t i = 0; i < count; i++) {
        const int32_t w = width[i], h0 = height[i], nints = (int32_t)(int_offsets[i + 1] - int_offsets[i]);
        const int32_t maxcuts = std::max(1, 2 * nints), hmax = h0 + 2 * nints;
        const MtTree T = {w, nints, integers + int_offsets[i], sign[i], precision[i], tolerance[i], maxIterations[i], timeout_ms[i] <= 0 ? 1 : 0};
        int64_t evaluated = 0;
        int32_t best_h = 0;
        MtState fin{};
        ncol0.assign((size_t)hmax, 0.0), npos.assign((size_t)w + hmax, 0), nvar.assign((size_t)w + hmax, 0);
        for (long long cap = arena;; cap *= 4) {
            if (cap > arena_max) {
                fin = MtState{};
                fin.status = YALPS_MILPTREE_OVERFLOW, fin.result = NAN;
                best_h = 0;
                seq_n.clear();
                break;
            }
            if (cap != arena) reruns++;
            mem.assign(mt_arena_doubles((int32_t)cap, maxcuts), 0.0);
            const MtArena A = mt_arena_bind(mem.data(), (int32_t)cap, maxcuts);
            seq_val.clear(), seq_eval.clear(), seq_sg.clear(), seq_vr.clear(), seq_n.clear();
            best_h = 0;
            mt_begin(T, A, root_status[i], root_result[i], root_col0 + c0, root_pos + p0);
            while (mt_next(T, A)) {
                const int32_t slot = A.state->cur_slot, nc = A.slot_n[slot], h = h0 + nc;
                sg.assign((size_t)nc, 0), vr.assign((size_t)nc, 0), vl.assign((size_t)nc, 0.0);
                for (int32_t q = 0; q < nc; q++) {
                    const size_t at = (size_t)slot * maxcuts + q;
                    sg[q] = A.cut_sv[2 * at], vr[q] = A.cut_sv[2 * at + 1], vl[q] = A.cut_val[at];
                }
                const int64_t coff[2] = {0, nc};
                int32_t st = YALPS_CYCLED, hg = 0;
                double rs = NAN;
                const int32_t rc = eval(user, 1, &i, coff, sg.data(), vr.data(), vl.data(), &st, &rs, &hg, ncol0.data(), npos.data(), nvar.data());
                if (rc < 0) return fail(rc, "yalps_milptree_search: the evaluator failed");
                if (st == YALPS_OPTIMAL && hg != h) return fail(YALPS_E_ARG, "yalps_milptree_search: the evaluator returned a node of another height");
                evaluated++;
                seq_eval.push_back(A.state->cur_eval), seq_n.push_back(nc);
                seq_sg.insert(seq_sg.end(), sg.begin(), sg.end()), seq_vr.insert(seq_vr.end(), vr.begin(), vr.end());
                seq_val.insert(seq_val.end(), vl.begin(), vl.end());
                if (mt_consume(T, A, st, rs, ncol0.data(), npos.data(), h) == MT_INCUMBENT) {
                    best_h = h;
                    std::memcpy(col0_out + oc0, ncol0.data(), sizeof(double) * (size_t)h);
                    std::memcpy(pos_out + op0, npos.data(), sizeof(int32_t) * ((size_t)w + h));
                    std::memcpy(var_out + op0, nvar.data(), sizeof(int32_t) * ((size_t)w + h));
                }
            }
            fin = *A.state;
            if (fin.status != MT_ARENA_FULL) break;
        }
        if (best_h == 0) { // bestTableau is the root's
            std::memcpy(col0_out + oc0, root_col0 + c0, sizeof(double) * (size_t)h0);
            std::memcpy(pos_out + op0, root_pos + p0, sizeof(int32_t) * ((size_t)w + h0));
            std::memcpy(var_out + op0, root_var + p0, sizeof(int32_t) * ((size_t)w + h0));
        }
        height_out[i] = best_h ? best_h : h0;
        if (status_out) status_out[i] = fin.status;
        if (result_out) result_out[i] = fin.result;
        if (stats_out) stats_out[2 * i] = fin.used, stats_out[2 * i + 1] = evaluated;
        if (consumed) {
            size_t c = 0;
            for (size_t k = 0; k < seq_n.size(); c += (size_t)seq_n[k], k++)
                consumed(user, i, seq_eval[k], seq_n[k], seq_sg.data() + c, seq_vr.data() + c, seq_val.data() + c);
        }
        c0 += (size_t)h0, p0 += (size_t)w + h0;
        oc0 += (size_t)hmax, op0 += (size_t)w + hmax;
    }
    if (reruns_out) *reruns_out = reruns;
    return 0;
}

int32_t yalps_milptree_info(const yalps_milptree *b, char *buf, int32_t len) {
    if (!b || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_milptree_info: bad argument");
    return info_out(b->info, buf, len);
}

} // extern "C"
