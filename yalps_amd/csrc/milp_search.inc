// milp_search.inc -- the search rules of branch and cut (src/branchAndCut.ts:64-85, :99-103, :141-158), host C++.
// Included by milp_host.inc (libyalps_hip.so: yalps_milp_f64, one tree at a time) and by milp_batch.hip
// (libyalps_milpbatch.so: many trees in lockstep): ONE statement of the queue order, of mostFractionalVar and of the two
// children's cut lists for both drivers.  Needs common.cuh (js_round) and the YALPS_* status codes.

namespace {

struct MilpCut {
    int32_t sign, variable;
    double value;
    bool operator<(const MilpCut &o) const {
        return sign != o.sign ? sign < o.sign : variable != o.variable ? variable < o.variable : value < o.value;
    }
};
using MilpCuts = std::vector<MilpCut>;

struct MilpBranch {
    double eval;
    MilpCuts cuts;
};

// heapq.heappush / heappop (CPython Lib/heapq.py): comparison on eval only
inline bool milp_lt(const MilpBranch &a, const MilpBranch &b) { return a.eval < b.eval; }
void milp_siftdown(std::vector<MilpBranch> &heap, size_t startpos, size_t pos) {
    MilpBranch newitem = std::move(heap[pos]);
    while (pos > startpos) {
        const size_t parentpos = (pos - 1) >> 1;
        if (milp_lt(newitem, heap[parentpos])) {
            heap[pos] = std::move(heap[parentpos]);
            pos = parentpos;
            continue;
        }
        break;
    }
    heap[pos] = std::move(newitem);
}
void milp_siftup(std::vector<MilpBranch> &heap, size_t pos) {
    const size_t endpos = heap.size(), startpos = pos;
    MilpBranch newitem = std::move(heap[pos]);
    size_t childpos = 2 * pos + 1;
    while (childpos < endpos) {
        const size_t rightpos = childpos + 1;
        if (rightpos < endpos && !milp_lt(heap[childpos], heap[rightpos])) childpos = rightpos;
        heap[pos] = std::move(heap[childpos]);
        pos = childpos;
        childpos = 2 * pos + 1;
    }
    heap[pos] = std::move(newitem);
    milp_siftdown(heap, startpos, pos);
}
void milp_push(std::vector<MilpBranch> &heap, MilpBranch item) {
    heap.push_back(std::move(item));
    milp_siftdown(heap, 0, heap.size() - 1);
}
MilpBranch milp_pop(std::vector<MilpBranch> &heap) {
    MilpBranch last = std::move(heap.back());
    heap.pop_back();
    if (heap.empty()) return last;
    MilpBranch ret = std::move(heap[0]);
    heap[0] = std::move(last);
    milp_siftup(heap, 0);
    return ret;
}

// what mostFractionalVar / solution() read of a solved tableau
struct MilpView {
    int32_t height = 0;
    std::vector<double> col0;
    std::vector<int32_t> pos, var;
};

struct MilpEval {
    int32_t status = YALPS_CYCLED;
    double result = NAN;
    MilpView view; // filled when status == optimal
};

// src/branchAndCut.ts:64-85
void milp_most_fractional(const MilpView &v, int32_t width, const int32_t *ints, int32_t nints, int32_t *variable, double *value,
                          double *frac_out) {
    double highest = 0.0, val_best = 0.0;
    int32_t var_best = 0;
    for (int32_t i = 0; i < nints; i++) {
        const int32_t row = v.pos[ints[i]] - width;
        if (row < 0) continue;
        const double val = v.col0[row];
        const double frac = std::fabs(val - js_round(val));
        if (frac > highest) {
            highest = frac;
            var_best = ints[i];
            val_best = val;
        }
    }
    *variable = var_best;
    *value = val_best;
    *frac_out = highest;
}

// :99-103: the root's two children
void milp_push_first(std::vector<MilpBranch> &branches, double root_result, int32_t variable, double value) {
    milp_push(branches, {root_result, {{-1, variable, std::ceil(value)}}});
    milp_push(branches, {root_result, {{1, variable, std::floor(value)}}});
}

// :137-158: the two children of node `br`, branched on `variable` at `value`, pushed with the node's own result
void milp_push_children(std::vector<MilpBranch> &branches, const MilpBranch &br, int32_t variable, double value, double result) {
    MilpCuts upper, lower;
    for (const MilpCut &cut : br.cuts) {
        if (cut.variable == variable) {
            (cut.sign < 0 ? lower : upper).push_back(cut);
        } else {
            upper.push_back(cut);
            lower.push_back(cut);
        }
    }
    lower.push_back({1, variable, std::floor(value)});
    upper.push_back({-1, variable, std::ceil(value)});
    milp_push(branches, {result, std::move(upper)});
    milp_push(branches, {result, std::move(lower)});
}

// the popped node's cuts first, then those of its next-best `node_batch - 1` frontier nodes (by evaluation, then by heap
// slot) that are neither in `cache` nor named twice: what one batch evaluates
template <class Cache>
std::vector<const MilpCuts *> milp_wanted(const std::vector<MilpBranch> &branches, const MilpCuts &first, int32_t node_batch,
                                          const Cache &cache) {
    std::vector<const MilpCuts *> todo{&first};
    std::vector<size_t> order(branches.size());
    for (size_t i = 0; i < order.size(); i++) order[i] = i;
    const size_t want = (size_t)node_batch - 1 < order.size() ? (size_t)node_batch - 1 : order.size();
    std::partial_sort(order.begin(), order.begin() + want, order.end(), [&](size_t a, size_t b2) {
        return branches[a].eval != branches[b2].eval ? branches[a].eval < branches[b2].eval : a < b2;
    });
    std::set<MilpCuts> seen{first};
    for (size_t k = 0; k < want; k++) {
        const MilpCuts &cs = branches[order[k]].cuts;
        if (cache.count(cs) || seen.count(cs)) continue;
        todo.push_back(&cs);
        seen.insert(cs);
    }
    return todo;
}

double milp_now_ms() {
    return (double)std::chrono::duration_cast<std::chrono::milliseconds>(std::chrono::system_clock::now().time_since_epoch()).count();
}

} // namespace
