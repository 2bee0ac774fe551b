// milp_host.inc -- native branch-and-cut driver (host C++), included at the end of yalps_hip.hip.
//
// yalps_milp_f64 = the reference's solve() flow for a model with integer variables, from the initial tableau to
// the best integer tableau, in ONE native call: simplex() on the root (src/YALPS.ts:79), then branchAndCut
// (src/branchAndCut.ts:89-176) with every node LP on the GPU.  The queue is a binary heap with CPython heapq's
// sift rules (the reference's queue is npm `heap`, package.json:157, described by its authors as a port of heapq), ordered
// by the parent's evaluation only (:100), so nodes are popped in the reference's order; results are committed in pop order.
// Node order is pinned to the reference's branchAndCut by tests/golden/simplex_milp.json.gz (a heapq stand-in for `heap`
// assumed, DESIGN.md section 2): tests/test_milp_paths.py checks every model's node count, best tableau and result.
// Node evaluation, by root size:
//   * root + cuts fit in LDS:        host-side applyCuts (:22-61) + the zero-copy single-workgroup solve
//                                    (or, node_batch > 1: batches of frontier nodes, one workgroup per node)
//   * up to 4 MB with node_batch > 1: batches in the HBM workspace (batch_kernel)
//   * otherwise:                     root resident in HBM, yalps_tableau_apply_cuts + solve per node
// A node's LP depends only on the root and its cuts, so evaluating frontier nodes early (batches) cannot change
// any result; checkCycles always takes the one-node-at-a-time paths.

// The queue (CPython heapq's sift rules), mostFractionalVar, the children's cut lists and the choice of the nodes of a
// batch are milp_search.inc: the lockstep driver of libyalps_milpbatch.so (milp_batch.hip) reads the same text.
#include "milp_search.inc"

extern "C" int32_t yalps_milp_f64(const double *matrix, int32_t width, int32_t height, const int32_t *positionOfVariable,
                       const int32_t *variableAtPosition, const int32_t *integers, int32_t n_integers, double sign,
                       double precision, double maxPivots, int32_t checkCycles, double tolerance, double timeout_ms,
                       double maxIterations, int32_t node_batch, int32_t *status_out, double *result_out, double *col0_out,
                       int32_t *pos_out, int32_t *var_out, int32_t *height_out, int64_t *stats_out) {
    if (!matrix || !positionOfVariable || !variableAtPosition || width < 1 || height < 1 || n_integers < 0 ||
        (n_integers > 0 && !integers) || !status_out || !result_out || !col0_out || !pos_out || !var_out || !height_out)
        return fail(YALPS_E_ARG, "yalps_milp_f64: bad argument");
    for (int32_t i = 0; i < n_integers; i++)
        if (integers[i] < 1 || integers[i] >= width) return fail(YALPS_E_ARG, "yalps_milp_f64: integer variable out of range");
    std::lock_guard<std::mutex> lock(g_default_mu);
    int32_t rc = default_ctx();
    if (rc) return rc;
    yalps_ctx *ctx = g_default_ctx;
    const int32_t max_cuts = 2 * n_integers, hmax = height + max_cuts;
    int64_t n_nodes = 0, n_evaluated = 0, n_batches = 0;

    // RAII for the device objects of this call
    struct Guard {
        yalps_tableau *root = nullptr, *node = nullptr;
        yalps_batch *batch = nullptr;
        ~Guard() {
            if (batch) yalps_batch_destroy(batch);
            if (node) yalps_tableau_destroy(node);
            if (root) yalps_tableau_destroy(root);
        }
    } g;

    // ---- root: simplex(tableau) (src/YALPS.ts:79), kept on the device ----
    rc = yalps_tableau_create(ctx, width, height, &g.root);
    if (rc) return rc;
    rc = yalps_tableau_upload(g.root, matrix, height, positionOfVariable, variableAtPosition);
    if (rc) return rc;
    double root_result = NAN;
    const int32_t root_status = yalps_tableau_solve(g.root, precision, maxPivots, checkCycles, &root_result, nullptr, nullptr);
    if (root_status < 0) return root_status;
    MilpView best;
    best.height = height;
    best.col0.resize((size_t)height);
    best.pos.resize((size_t)width + height);
    best.var.resize((size_t)width + height);
    rc = yalps_tableau_download_solution(g.root, best.col0.data(), best.pos.data(), best.var.data());
    if (rc) return rc;
    auto finish = [&](int32_t status, double result) {
        *status_out = status;
        *result_out = result;
        *height_out = best.height;
        std::memcpy(col0_out, best.col0.data(), sizeof(double) * (size_t)best.height);
        std::memcpy(pos_out, best.pos.data(), sizeof(int32_t) * ((size_t)width + best.height));
        std::memcpy(var_out, best.var.data(), sizeof(int32_t) * ((size_t)width + best.height));
        if (stats_out) {
            stats_out[0] = n_nodes;
            stats_out[1] = n_evaluated;
            stats_out[2] = n_batches;
        }
        return 0;
    };
    if (root_status != YALPS_OPTIMAL || n_integers == 0) return finish(root_status, root_result);

    int32_t variable = 0;
    double value = 0.0, frac = 0.0;
    milp_most_fractional(best, width, integers, n_integers, &variable, &value, &frac);
    if (frac <= precision) return finish(YALPS_OPTIMAL, root_result); // :94-95

    // ---- how nodes are evaluated ----
    const size_t root_bytes = sizeof(double) * (size_t)width * height;
    const bool lds_nodes = fits_small(ctx, width, hmax);
    const bool batched = node_batch > 1 && !checkCycles && root_bytes <= ((size_t)4 << 20);
    const bool host_nodes = lds_nodes && !batched; // host applyCuts + zero-copy small_kernel per node
    std::vector<double> root_matrix;               // the root's optimal tableau on the host (host applyCuts, batches)
    std::vector<double> node_matrix;
    std::vector<int32_t> node_pos, node_var;
    if (host_nodes || batched) {
        root_matrix.resize((size_t)width * height);
        rc = yalps_tableau_download(g.root, root_matrix.data(), nullptr, nullptr);
        if (rc) return rc;
    }
    if (host_nodes) {
        node_matrix.resize((size_t)width * hmax);
        node_pos.resize((size_t)width + hmax);
        node_var.resize((size_t)width + hmax);
    } else if (batched) {
        rc = yalps_batch_create(ctx, width, height, max_cuts > 0 ? max_cuts : 1, node_batch, &g.batch);
        if (rc) return rc;
        rc = yalps_batch_set_root(g.batch, root_matrix.data(), best.pos.data(), best.var.data());
        if (rc) return rc;
    } else {
        rc = yalps_tableau_create(ctx, width, hmax, &g.node);
        if (rc) return rc;
    }
    const MilpView root_view = best; // (positions of the root: applyCuts reads them)
    std::vector<int32_t> c_sign, c_var;
    std::vector<double> c_val;

    // one node, now
    auto evaluate_one = [&](const MilpCuts &cuts, MilpEval *out) -> int32_t {
        const int32_t nc = (int32_t)cuts.size(), h = height + nc;
        n_evaluated++;
        if (host_nodes) { // applyCuts on the host (:22-61), then the drop-in call (pinned zero-copy path)
            std::memcpy(node_matrix.data(), root_matrix.data(), sizeof(double) * root_matrix.size());
            for (int32_t i = 0; i < nc; i++) {
                double *row = node_matrix.data() + (size_t)(height + i) * width;
                const double s = (double)cuts[i].sign;
                const int32_t p = root_view.pos[cuts[i].variable];
                if (p < width) {
                    row[0] = s * cuts[i].value;
                    for (int32_t c = 1; c < width; c++) row[c] = 0.0;
                    row[p] = s;
                } else {
                    const double *src = root_matrix.data() + (size_t)(p - width) * width;
                    row[0] = s * (cuts[i].value - src[0]);
                    for (int32_t c = 1; c < width; c++) row[c] = -s * src[c];
                }
            }
            for (int32_t k = 0; k < width + height; k++) {
                node_pos[k] = root_view.pos[k];
                node_var[k] = root_view.var[k];
            }
            for (int32_t k = width + height; k < width + h; k++) node_pos[k] = node_var[k] = k;
            const int32_t st = simplex_f64_locked(node_matrix.data(), width, h, node_pos.data(), node_var.data(), precision,
                                                  maxPivots, checkCycles, YALPS_COPYBACK_SOLUTION, &out->result, nullptr);
            if (st < 0) return st;
            out->status = st;
            if (st == YALPS_OPTIMAL) {
                out->view.height = h;
                out->view.col0.resize((size_t)h);
                for (int32_t r = 0; r < h; r++) out->view.col0[r] = node_matrix[(size_t)r * width];
                out->view.pos.assign(node_pos.begin(), node_pos.begin() + width + h);
                out->view.var.assign(node_var.begin(), node_var.begin() + width + h);
            }
            return 0;
        }
        c_sign.resize((size_t)nc);
        c_var.resize((size_t)nc);
        c_val.resize((size_t)nc);
        for (int32_t i = 0; i < nc; i++) {
            c_sign[i] = cuts[i].sign;
            c_var[i] = cuts[i].variable;
            c_val[i] = cuts[i].value;
        }
        // column 0 and the permutations ride along with the solve's own wait where the persistent path allows it
        out->view.height = h;
        out->view.col0.resize((size_t)h);
        out->view.pos.resize((size_t)width + h);
        out->view.var.resize((size_t)width + h);
        // (one call: three launches and one wait where the node takes the resident kernel, else call by call)
        const int32_t st = yalps_tableau_node_solve(g.node, g.root, nc, c_sign.data(), c_var.data(), c_val.data(), precision, maxPivots,
                                                    checkCycles, &out->result, out->view.col0.data(), out->view.pos.data(),
                                                    out->view.var.data());
        if (st < 0) return st;
        out->status = st;
        return 0;
    };

    std::vector<MilpBranch> branches; // :99-103
    milp_push_first(branches, root_result, variable, value);
    std::map<MilpCuts, MilpEval> cache; // batched: results of nodes evaluated ahead of their turn
    std::vector<double> bulk_col0;
    std::vector<int32_t> bulk_pos, bulk_var;

    // the popped node together with the next-best frontier nodes, one workgroup per node
    auto evaluate_batch = [&](const MilpCuts &first) -> int32_t {
        const std::vector<const MilpCuts *> todo = milp_wanted(branches, first, node_batch, cache);
        const int32_t count = (int32_t)todo.size();
        std::vector<int32_t> off((size_t)count + 1, 0), sg, vr, st((size_t)count);
        std::vector<double> vl, res((size_t)count);
        for (int32_t i = 0; i < count; i++) {
            for (const MilpCut &cut : *todo[i]) {
                sg.push_back(cut.sign);
                vr.push_back(cut.variable);
                vl.push_back(cut.value);
            }
            off[i + 1] = (int32_t)sg.size();
        }
        if (sg.empty()) {
            sg.push_back(0);
            vr.push_back(0);
            vl.push_back(0.0);
        }
        // cuts up, one workgroup per node, and every node's status / result / column 0 / permutations back: one wait
        const BatchDesc &bd = g.batch->d;
        bulk_col0.resize((size_t)count * bd.hmax);
        bulk_pos.resize((size_t)count * bd.permmax);
        bulk_var.resize((size_t)count * bd.permmax);
        const int32_t r2 = batch_solve_fetch(g.batch, count, off.data(), sg.data(), vr.data(), vl.data(), precision, maxPivots,
                                             st.data(), res.data(), bulk_col0.data(), bulk_pos.data(), bulk_var.data());
        if (r2) return r2;
        n_batches++;
        n_evaluated += count;
        for (int32_t i = 0; i < count; i++) {
            MilpEval ev;
            ev.status = st[i];
            ev.result = res[i];
            if (st[i] == YALPS_OPTIMAL) {
                const int32_t h = height + (off[i + 1] - off[i]);
                ev.view.height = h;
                ev.view.col0.assign(bulk_col0.begin() + (size_t)i * bd.hmax, bulk_col0.begin() + (size_t)i * bd.hmax + h);
                ev.view.pos.assign(bulk_pos.begin() + (size_t)i * bd.permmax, bulk_pos.begin() + (size_t)i * bd.permmax + width + h);
                ev.view.var.assign(bulk_var.begin() + (size_t)i * bd.permmax, bulk_var.begin() + (size_t)i * bd.permmax + width + h);
            }
            cache.emplace(*todo[i], std::move(ev));
        }
        return 0;
    };

    // ---- :105-164 ----
    const double optimal_threshold = root_result * (1.0 - sign * tolerance);
    const double stop_time = timeout_ms + milp_now_ms();
    bool timedout = milp_now_ms() >= stop_time, solution_found = false;
    double best_eval = INFINITY, iter = 0.0;
    while (iter < maxIterations && !branches.empty() && best_eval >= optimal_threshold && !timedout) {
        MilpBranch br = milp_pop(branches);
        if (br.eval > best_eval) break; // :119
        MilpEval ev;
        if (batched) {
            auto it = cache.find(br.cuts);
            if (it == cache.end()) {
                rc = evaluate_batch(br.cuts);
                if (rc) return rc;
                it = cache.find(br.cuts);
            }
            ev = std::move(it->second);
            cache.erase(it);
        } else {
            rc = evaluate_one(br.cuts, &ev);
            if (rc) return rc;
        }
        n_nodes++;
        if (ev.status == YALPS_OPTIMAL && ev.result < best_eval) {
            milp_most_fractional(ev.view, width, integers, n_integers, &variable, &value, &frac);
            if (frac <= precision) { // :131-136
                solution_found = true;
                best_eval = ev.result;
                best = std::move(ev.view);
            } else { // :137-158
                milp_push_children(branches, br, variable, value, ev.result);
            }
        }
        timedout = milp_now_ms() >= stop_time;
        iter += 1.0;
    }
    const bool unfinished = (timedout || iter >= maxIterations) && !branches.empty() && best_eval >= optimal_threshold; // :166-173
    const int32_t status = unfinished ? 4 /* timedout */ : (solution_found ? YALPS_OPTIMAL : YALPS_INFEASIBLE);
    return finish(status, solution_found ? best_eval : NAN);
}
