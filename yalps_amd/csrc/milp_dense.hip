// milp_dense.hip -- libyalps_milpdense.so: a batch of dense MILPs of one shape, from device operands to device answers, every
// branch-and-cut tree walked on the device (include/yalps_milpdense.h).  C ABI, host side, and three device parts:
// milp_dense_root_kernel (milp_dense_kernel.cuh: lp_dense_kernel's job plus the binary rows, tableaux kept),
// milp_tree_kernel (milp_tree_kernel.cuh, unchanged, on the pass / rerun / arena protocol of milp_tree_host.inc, which
// libyalps_milptree.so runs too) and milp_dense_solution_kernel (solution() of every tree into dense rows).
// A library of its own: nothing here is linked into the others.  Nothing of a MILP crosses PCIe but its status: the operands
// are read where they lie, x / objective are written by the epilogue, status and counts are copied device to device, and the
// best tableaux stay on the device until yalps_milpdense_solution asks for one.
// A call with bounds (lb / ub) runs milp_dense_bounds_root_kernel and milp_dense_bounds_solution_kernel
// (milp_dense_bounds_kernel.cuh), whose forms are libyalps_milpdense_bounds.so's: this library links it and takes the kernels'
// pointers from yalps_milpdense_bounds_forms, so its own code object holds the boundless kernels alone.
// A call with free variables (n_free > 0) runs milp_dense_free_root_kernel and milp_dense_free_solution_kernel
// (milp_dense_free_kernel.cuh) on a tableau n_free columns wider, the kernels of libyalps_milpdense_free.so, linked likewise;
// milp_tree_kernel is given the twin columns of the free integer variables behind the integer variables' own.
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

#include "../../include/yalps_milpdense.h"

#pragma clang fp contract(off)

#include "milp_tree_rules.cuh"

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_batch_kernel.cuh" // (LpDesc: what milp_tree_kernel reads of a root; lp_batch_kernel itself is not instantiated here)
#include "milp_tree_kernel.cuh"
#include "milp_dense_kernel.cuh"
#include "milp_dense_bounds_kernel.cuh" // (the siblings' kernels, for their types; they are not instantiated here)
#include "milp_dense_free_kernel.cuh"
#include "wg_queue_host.inc"
#include "milp_tree_host.inc"
#include "dense_host.inc"

static_assert(YALPS_MILPDENSE_MAX_BYTES == QUEUE_MAX_BYTES, "include/yalps_milpdense.h");
static_assert(TREE_TIMEDOUT == YALPS_MILPDENSE_TIMEDOUT && TREE_OVERFLOW == YALPS_MILPDENSE_OVERFLOW, "include/yalps_milpdense.h");
const KernelTable<MilpDenseLaunch> kRootKernels = QUEUE_KERNEL_TABLE(milp_dense_root_kernel);
constexpr int SOLUTION_LANES = 256;
struct X { // (dense_host.inc)
    static constexpr const char *name = "yalps_milpdense";
    using Operand = yalps_milpdense_operand;
};
} // namespace

extern "C" void yalps_milpdense_bounds_forms(void *out[7]); // milp_dense_bounds.hip
extern "C" void yalps_milpdense_free_forms(void *out[7]);   // milp_dense_free.hip

namespace {
// a sibling library's kernels: the same table over its root forms, and its epilogue
struct SiblingKernels {
    KernelTable<MilpDenseLaunch> roots;
    void (*solution)(MilpSolutionArgs);
};
SiblingKernels sibling(const char *name, void (*forms)(void **)) {
    void *solution = nullptr;
    SiblingKernels k{adopt_forms(kRootKernels, name, forms, &solution), nullptr};
    k.solution = reinterpret_cast<void (*)(MilpSolutionArgs)>(solution);
    return k;
}
const SiblingKernels &bounds_kernels() { // libyalps_milpdense_bounds.so's
    static const SiblingKernels kernels = sibling("milp_dense_bounds_root_kernel", yalps_milpdense_bounds_forms);
    return kernels;
}
const SiblingKernels &free_kernels() { // libyalps_milpdense_free.so's
    static const SiblingKernels kernels = sibling("milp_dense_free_root_kernel", yalps_milpdense_free_forms);
    return kernels;
}
} // namespace

struct yalps_milpdense : QueueDevice {
    QueueBufs q;                  // the root pass
    QueueDevice root;             // the root pass's class table: the handle's own, but for the test hooks _CUS / _PER_CU
    DevBuf call, rdesc;           // the call's description with the binary list behind it; one LpDesc per root
    TreePass t;
    // the last solve
    std::vector<LpDesc> roots;
    int32_t n = 0, w = 0, h0 = 0, nints = 0, count = 0; // nints: the integer COLUMNS, the twins of free integer variables among them
    bool walked = false;          // there was a tree pass
    std::vector<int32_t> overflowed;
    std::string info;
};

namespace {
// a HOST list of 0-based variable indices: strictly ascending, within 0 .. n - 1
int check_list(const char *name, int32_t len, const int32_t *list, int32_t n) {
    const std::string who = std::string("yalps_milpdense: ") + name;
    if (len < 0) return fail(YALPS_E_ARG, who + ": negative length");
    if (len > 0 && !list) return fail(YALPS_E_ARG, who + " is NULL");
    for (int32_t k = 0; k < len; k++) {
        if (list[k] < 0 || list[k] >= n) return fail(YALPS_E_ARG, who + ": variable " + std::to_string(list[k]) + " out of range");
        if (k > 0 && list[k] <= list[k - 1]) return fail(YALPS_E_ARG, who + " is not strictly ascending at variable " + std::to_string(list[k]));
    }
    return 0;
}

int validate(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
             const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq, int32_t nints,
             const int32_t *ints, int32_t nbin, const int32_t *bin, int32_t n_upper = 0, int32_t n_free = 0, int32_t int_twins = 0) {
    if (count < 0) return fail(YALPS_E_ARG, "yalps_milpdense: count < 0");
    if (n < 0 || m_ub < 0 || m_eq < 0) return fail(YALPS_E_ARG, "yalps_milpdense: n, m_ub and m_eq must be at least 0");
    if (n_upper < 0) return fail(YALPS_E_ARG, "yalps_milpdense: n_upper < 0");
    if (int rc = check_list("integers", nints, ints, n)) return rc;
    if (int rc = check_list("binaries", nbin, bin, n)) return rc;
    for (int32_t k = 0, at = 0; k < nbin; k++) { // (both ascending: one walk)
        while (at < nints && ints[at] < bin[k]) at++;
        if (at >= nints || ints[at] != bin[k])
            return fail(YALPS_E_ARG, "yalps_milpdense: binary variable " + std::to_string(bin[k]) + " is not in integers (the union of both sets)");
    }
    const int64_t w = (int64_t)n + 1 + n_free, h = 1 + (int64_t)m_ub + 2 * (int64_t)m_eq + (int64_t)n_upper + nbin;
    const int64_t hmax = h + 2 * ((int64_t)nints + int_twins);
    if (n_free > 0 && (w > INT32_MAX || hmax > INT32_MAX || 8 * w * hmax > YALPS_MILPDENSE_MAX_BYTES))
        return fail(YALPS_E_ARG, "yalps_milpdense: largest node of " + std::to_string(hmax) + " x " + std::to_string(w) + " doubles (" +
                                     std::to_string(n_free) + " twin columns of free variables, " + std::to_string(h) +
                                     " rows and two cuts for each of " + std::to_string(nints + int_twins) + " integer columns: " +
                                     std::to_string(nints) + " integer variables and the twins of the " + std::to_string(int_twins) +
                                     " free ones among them) is above the limit of " + std::to_string((long long)YALPS_MILPDENSE_MAX_BYTES) + " bytes");
    if (w > INT32_MAX || hmax > INT32_MAX || 8 * w * hmax > YALPS_MILPDENSE_MAX_BYTES)
        return fail(YALPS_E_ARG, "yalps_milpdense: largest node of " + std::to_string(hmax) + " x " + std::to_string(w) + " doubles (" +
                                     std::to_string(h) + " rows and two cuts for each of " + std::to_string(nints) +
                                     " integer variables) is above the limit of " + std::to_string((long long)YALPS_MILPDENSE_MAX_BYTES) + " bytes");
    return check_operands<X>(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq);
}

// the bounds of a call: lb / ub may be NULL descriptors (absent); upper_idx is host memory, ascending, inside 0 .. n-1, and names
// no binary variable (yalps_lpdense_validate_bounds' refusals, by the same words, and that one)
int validate_bounds(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                    const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq,
                    const yalps_milpdense_operand *lb, const yalps_milpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx,
                    int32_t nints, const int32_t *ints, int32_t nbin, const int32_t *bin, int32_t n_free = 0, int32_t int_twins = 0) {
    if (int rc = validate(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, nints, ints, nbin, bin, n_upper, n_free, int_twins)) return rc;
    int32_t at = 0; // (both ascending: one walk)
    return check_bounds<X>(count, n, lb, ub, n_upper, upper_idx, [&](int32_t t) {
        while (at < nbin && bin[at] < upper_idx[t]) at++;
        if (at < nbin && bin[at] == upper_idx[t])
            return fail(YALPS_E_ARG, "yalps_milpdense: upper_idx[" + std::to_string(t) + "]: variable " + std::to_string(upper_idx[t]) +
                                         " is binary (a binary variable has no bound row)");
        return 0;
    });
}

// the free variables of a call: free_idx is host memory, strictly ascending, inside 0 .. n-1, and names no binary variable; the
// width counts the n_free twins, the largest node the two cuts of every twin of a free INTEGER variable too.  *int_twins_out:
// their number.  n_free = 0: validate_bounds.
int validate_free(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                  const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq,
                  const yalps_milpdense_operand *lb, const yalps_milpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx,
                  int32_t n_free, const int32_t *free_idx, int32_t nints, const int32_t *ints, int32_t nbin, const int32_t *bin,
                  int32_t *int_twins_out = nullptr) {
    int32_t int_twins = 0;
    if (n_free != 0) {
        if (n < 0) return fail(YALPS_E_ARG, "yalps_milpdense: n, m_ub and m_eq must be at least 0");
        if (int rc = check_list("integers", nints, ints, n)) return rc;
        if (int rc = check_list("binaries", nbin, bin, n)) return rc;
        if (int rc = check_list("free_idx", n_free, free_idx, n)) return rc;
        for (int32_t t = 0, at = 0, ai = 0; t < n_free; t++) { // (all three ascending: one walk)
            while (at < nbin && bin[at] < free_idx[t]) at++;
            if (at < nbin && bin[at] == free_idx[t])
                return fail(YALPS_E_ARG, "yalps_milpdense: free_idx[" + std::to_string(t) + "]: variable " + std::to_string(free_idx[t]) +
                                             " is binary (a binary variable cannot be free)");
            while (ai < nints && ints[ai] < free_idx[t]) ai++;
            if (ai < nints && ints[ai] == free_idx[t]) int_twins++;
        }
    }
    if (int_twins_out) *int_twins_out = int_twins;
    return validate_bounds(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, lb, ub, n_upper, upper_idx, nints, ints, nbin, bin, n_free, int_twins);
}

int create_impl(int32_t device, void *hip_stream, yalps_milpdense **out) {
    yalps_milpdense *b = new yalps_milpdense();
    *out = b;
    // (test hooks: the ROOT pass on a grid smaller than the card, one per_cu for every class, so that a workgroup takes several
    // roots of any class; read and refused in front of the device, 0 or unset: the card's own table.  The trees keep _GRID.)
    const int per_cu = env_int("YALPS_MILPDENSE_PER_CU", 0), cus = env_int("YALPS_MILPDENSE_CUS", 0);
    if (per_cu < 0 || per_cu > 8) return fail(YALPS_E_ARG, "YALPS_MILPDENSE_PER_CU: " + std::to_string(per_cu) + " is outside 0..8 (0: unset)");
    if (cus < 0) return fail(YALPS_E_ARG, "YALPS_MILPDENSE_CUS: " + std::to_string(cus) + " is negative");
    if (int rc = open_device(*b, device, hip_stream)) return rc;
    if (hip_stream == static_cast<void *>(hipStreamLegacy)) b->stream = nullptr; // the device's default stream, by its own name
    b->root = *b; // (the same stream and events: one pass runs at a time)
    if (cus) b->root.num_cus = std::min(cus, b->num_cus);
    if (per_cu)
        for (int k = 0; k < NCLASS; k++) b->root.per_cu[k] = std::min(per_cu, kClasses[k].per_cu);
    b->q.hist_first = b->t.q.hist_first = std::max(1, env_int("YALPS_MILPDENSE_HIST", (int)HIST_FIRST)); // (test hooks: they force the reruns)
    b->t.arena_first = std::max(2, env_int("YALPS_MILPDENSE_ARENA", ARENA_FIRST));
    b->t.arena_max = std::max(2, env_int("YALPS_MILPDENSE_ARENA_MAX", ARENA_MAX));
    b->t.grid = std::max(0, env_int("YALPS_MILPDENSE_GRID", 0));
    b->info = "launches=0 reruns=0 overflows=0 gpu_us=0 root_us=0 tree_us=0 epilogue_us=0 rerun_lps=[] rerun_trees=[]\n";
    if (int rc = raise_lds_limit(kRootKernels)) return rc;
    if (int rc = raise_lds_limit(bounds_kernels().roots)) return rc;
    if (int rc = raise_lds_limit(free_kernels().roots)) return rc;
    return raise_lds_limit(kTreeKernels);
}

struct Times {
    float root = 0.f, epilogue = 0.f;
    int launches = 0;
    std::vector<int32_t> rerun_lps;
    std::string root_lines, epilogue_line;
};

int solve_impl(yalps_milpdense *b, const char *entry, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c,
               const yalps_milpdense_operand *A_ub, const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq,
               const yalps_milpdense_operand *b_eq, int32_t nints, const int32_t *ints, int32_t nbin, const int32_t *bin,
               int32_t maximize, double precision, double maxPivots, int32_t checkCycles, double tolerance, double maxIter,
               int32_t trace_cap, double *x_out, double *objective_out, int32_t *status_out, int64_t *nodes_out,
               int64_t *node_pivots_out, int64_t *root_pivots_out, Times &tm, const yalps_milpdense_operand *lb = nullptr,
               const yalps_milpdense_operand *ub = nullptr, int32_t n_upper = 0, const int32_t *upper_idx = nullptr, int32_t n_free = 0,
               const int32_t *free_idx = nullptr) {
    TreePass &t = b->t;
    const bool split = n_free > 0; // (any free variable: the free kernels, with or without bounds)
    const bool bounds = lb || ub;  // (else either descriptor: the bounded kernels; neither: the kernels and the bits of before)
    const bool lists = split || bounds; // the bound rows' index list and the kind bytes are uploaded
    b->count = 0;
    b->walked = false;
    b->overflowed.clear();
    t.trees.clear();
    t.lines.clear();
    t.rerun_ids.clear();
    t.launches = t.overflows = 0;
    t.gpu_ms = 0.0;
    if (trace_cap < 0) return fail(YALPS_E_ARG, std::string(entry) + ": trace_cap < 0");
    int32_t int_twins = 0;
    if (int rc = validate_free(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, lb, ub, n_upper, upper_idx, n_free, free_idx, nints, ints, nbin, bin,
                               &int_twins))
        return rc;
    if (count == 0) return 0;
    HIP_TRY(hipSetDevice(b->device));
    const struct {
        const char *name;
        const void *p;
    } pointers[] = {{"c", n ? c->ptr : nullptr},
                    {"A_ub", m_ub && n ? A_ub->ptr : nullptr},
                    {"b_ub", m_ub ? b_ub->ptr : nullptr},
                    {"A_eq", m_eq && n ? A_eq->ptr : nullptr},
                    {"b_eq", m_eq ? b_eq->ptr : nullptr},
                    {"lb", lb && n ? lb->ptr : nullptr},
                    {"ub", ub && n_upper ? ub->ptr : nullptr},
                    {"x_out", n ? x_out : nullptr},
                    {"objective_out", objective_out},
                    {"status_out", status_out},
                    {"nodes_out", nodes_out},
                    {"node_pivots_out", node_pivots_out},
                    {"root_pivots_out", root_pivots_out}};
    for (const auto &a : pointers)
        if (int rc = check_pointer(b->device, entry, a.name, a.p)) return rc;

    hipStream_t s = b->stream;
    const int32_t cols_n = nints + int_twins; // n_int_eff: the integer columns the trees branch on
    const int32_t w = n + 1 + n_free, h = 1 + m_ub + 2 * m_eq + n_upper + nbin, hmax = h + 2 * cols_n;
    const size_t cnt = (size_t)count, heven = ((size_t)h + 1) & ~(size_t)1, perm = (size_t)w + (size_t)h;
    const bool aux = lp_class(w, h) == HBM_CLASS && lp_aux_hbm(w, h);

    // ---- the root pass: the description and the binary list behind it, one launch per pass, tableaux kept for the trees
    // (a bounded call: more of the description, and behind the binary list the bound rows' index list and the kind bytes; a call
    // with free variables: all of it, and behind the kind bytes, from the next multiple of 4, free_idx and twin)
    const size_t desc_bytes = dense_desc_bytes(bounds, split);
    const size_t call_bytes = (desc_bytes + 15) & ~(size_t)15;
    const size_t bin_bytes = sizeof(int32_t) * (size_t)nbin, idx_bytes = sizeof(int32_t) * (size_t)n_upper;
    const size_t kind_bytes = ((size_t)n + 3) & ~(size_t)3, free_bytes = sizeof(int32_t) * (size_t)n_free, twin_bytes = sizeof(int32_t) * (size_t)n;
    if (int rc = ensure(b->call, call_bytes + bin_bytes + (lists ? idx_bytes + (split ? kind_bytes + free_bytes + twin_bytes : (size_t)n) : 0))) return rc;
    b->q.keep = true;
    if (int rc = ensure_outputs(b->q, cnt, heven * cnt, perm * cnt, (size_t)w * (size_t)h * cnt)) return rc;
    DenseDesc D{};
    D.n = n, D.m_ub = m_ub, D.m_eq = m_eq, D.n_bin = nbin;
    D.aux_hbm = aux ? 1 : 0;
    D.sign = maximize ? 1.0 : -1.0;
    D.precision = precision;
    D.max_pivots = maxPivots;
    D.c = operand(c, true);
    D.A_ub = operand(A_ub, false);
    D.b_ub = operand(b_ub, true);
    D.A_eq = operand(A_eq, false);
    D.b_eq = operand(b_eq, true);
    D.bin = reinterpret_cast<const int32_t *>(b->call.as<char>() + call_bytes);
    std::vector<uint8_t> kinds; // 0 continuous, 1 integer, 2 binary
    std::vector<int32_t> twins; // the twin's column of a free variable, -1 of any other
    if (lists) {
        if (lb && n) D.lb = operand(lb, true);
        if (ub && n_upper) D.ub = operand(ub, true);
        D.n_upper = n_upper;
        char *behind = b->call.as<char>() + call_bytes + bin_bytes;
        D.upper_idx = reinterpret_cast<const int32_t *>(behind);
        D.kind = reinterpret_cast<const uint8_t *>(behind + idx_bytes);
        kinds.assign((size_t)n, 0);
        for (int32_t k = 0; k < nints; k++) kinds[(size_t)ints[k]] = 1;
        for (int32_t k = 0; k < nbin; k++) kinds[(size_t)bin[k]] = 2;
        if (n_upper) HIP_TRY(hipMemcpyAsync(behind, upper_idx, idx_bytes, hipMemcpyHostToDevice, s));
        if (n) HIP_TRY(hipMemcpyAsync(behind + idx_bytes, kinds.data(), (size_t)n, hipMemcpyHostToDevice, s));
        if (split) {
            char *lists_at = behind + idx_bytes + kind_bytes;
            D.n_free = n_free;
            D.free_idx = reinterpret_cast<const int32_t *>(lists_at);
            D.twin = reinterpret_cast<const int32_t *>(lists_at + free_bytes);
            twins.assign((size_t)n, -1);
            for (int32_t k = 0; k < n_free; k++) twins[(size_t)free_idx[k]] = 1 + n + k;
            HIP_TRY(hipMemcpyAsync(lists_at, free_idx, free_bytes, hipMemcpyHostToDevice, s));
            HIP_TRY(hipMemcpyAsync(lists_at + free_bytes, twins.data(), twin_bytes, hipMemcpyHostToDevice, s));
        }
    }
    HIP_TRY(hipMemcpyAsync(b->call.p, &D, desc_bytes, hipMemcpyHostToDevice, s));
    if (nbin) HIP_TRY(hipMemcpyAsync(b->call.as<char>() + call_bytes, bin, bin_bytes, hipMemcpyHostToDevice, s));
    if (int rc = reset_status(b->q, s, cnt)) return rc;
    HIP_TRY(hipStreamSynchronize(s)); // (D, kinds and twins are on this frame, `bin`, `upper_idx` and `free_idx` are the caller's)
    b->n = n, b->w = w, b->h0 = h, b->nints = cols_n;

    QueueRun run;
    const int rc = run_queue(
        b->root, b->q, split ? free_kernels().roots : bounds ? bounds_kernels().roots : kRootKernels, QueueText{"yalps_milpdense", true, entry, "MILP"}, cnt,
        [&](int32_t, int *iw, int *ih) { return *iw = w, *ih = h, checkCycles != 0; },
        [&](MilpDenseLaunch &a) { a.call = b->call.as<const DenseDesc>(); }, [] { return 0; },
        [&](const Launch &L, const std::string &kernel, int pass, int launch, long long hist_cap) {
            char line[256];
            std::snprintf(line, sizeof line, "launch=%d pass=%d kernel=%s class=%d aux=%d lps=%zu grid=%d lds=%zu hist_cap=%lld\n", launch,
                          pass, kernel.c_str(), L.cls, aux ? 1 : 0, L.items.size(), L.grid, L.shmem, hist_cap);
            tm.root_lines += line;
        },
        run);
    if (rc) return rc;
    tm.root = run.ms;
    tm.launches = run.launches;
    tm.rerun_lps = run.reruns;
    t.launches = run.launches; // (the tree pass numbers its launches on from here)

    // ---- the tree pass: every tree is root i of the one shape
    const bool walk = nints > 0;
    if (walk) {
        std::vector<LpDesc> &R = b->roots;
        std::vector<TreeDesc> T(cnt);
        R.resize(cnt);
        const int32_t maxcuts = std::max(1, 2 * cols_n), cls = lp_class(w, hmax);
        const size_t tree_col0 = ((size_t)hmax + 1) & ~(size_t)1, tree_perm = (size_t)w + (size_t)hmax;
        const size_t tree_trace = (size_t)trace_cap * (4 + 2 * (size_t)maxcuts);
        for (size_t i = 0; i < cnt; i++) {
            LpDesc &r = R[i];
            r = LpDesc{};
            r.w = w, r.h = h;
            r.col0_off = (long long)(i * heven), r.perm_off = (long long)(i * perm), r.tab_off = (long long)(i * (size_t)w * (size_t)h);
            r.precision = precision, r.max_pivots = maxPivots;
            r.aux_hbm = aux ? 1 : 0;
            TreeDesc &d = T[i];
            d = TreeDesc{};
            d.nints = cols_n, d.maxcuts = maxcuts;
            d.ints_off = 0; // (one list for the whole call)
            d.sign = D.sign, d.tolerance = tolerance, d.max_iter = maxIter;
            d.timedout = 0;
            d.cls = cls;
            d.col0_off = (long long)(i * tree_col0), d.perm_off = (long long)(i * tree_perm), d.trace_off = (long long)(i * tree_trace);
            d.aux_hbm = lp_aux_hbm(w, hmax) ? 1 : 0;
        }
        // the tableau's integer columns: variable j is column j + 1; behind them the twins of the free integer variables in
        // ascending j (every twin's column is above n), so the whole list ascends
        std::vector<int32_t> cols((size_t)nints);
        for (int32_t k = 0; k < nints; k++) cols[(size_t)k] = ints[k] + 1;
        if (split)
            for (int32_t k = 0; k < nints; k++)
                if (twins[(size_t)ints[k]] >= 0) cols.push_back(twins[(size_t)ints[k]]);
        t.q.keep = false;
        t.trace_cap = trace_cap;
        if (int rc2 = ensure(b->rdesc, sizeof(LpDesc) * cnt)) return rc2;
        if (int rc2 = ensure(t.tdesc, sizeof(TreeDesc) * cnt)) return rc2;
        if (int rc2 = ensure(t.ints, sizeof(int32_t) * cols.size())) return rc2;
        if (int rc2 = ensure(t.d_used, sizeof(long long) * cnt)) return rc2;
        if (int rc2 = ensure(t.d_best_h, sizeof(int32_t) * cnt)) return rc2;
        if (int rc2 = ensure(t.d_trace, sizeof(double) * tree_trace * cnt)) return rc2;
        if (int rc2 = ensure_outputs(t.q, cnt, tree_col0 * cnt, tree_perm * cnt, 0)) return rc2;
        HIP_TRY(hipMemcpyAsync(b->rdesc.p, R.data(), sizeof(LpDesc) * cnt, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t.tdesc.p, T.data(), sizeof(TreeDesc) * cnt, hipMemcpyHostToDevice, s));
        HIP_TRY(hipMemcpyAsync(t.ints.p, cols.data(), sizeof(int32_t) * cols.size(), hipMemcpyHostToDevice, s));
        if (int rc2 = reset_status(t.q, s, cnt)) return rc2;
        HIP_TRY(hipStreamSynchronize(s)); // (T and cols are on this frame)
        t.trees = std::move(T);
        const TreeRoots roots{b, R.data(), b->rdesc.as<const LpDesc>(), &b->q};
        if (int rc2 = trees_impl(&t, roots, cnt, [&](int32_t) { return checkCycles != 0; }, "yalps_milpdense")) return rc2;
        for (size_t i = 0; i < cnt; i++)
            if (t.q.h_status[i] == TREE_OVERFLOW) b->overflowed.push_back((int32_t)i);
    }

    // ---- the epilogue: status and counts device to device, then solution() of every tree
    const QueueBufs &last = walk ? t.q : b->q;
    if (status_out) HIP_TRY(hipMemcpyAsync(status_out, last.status.p, sizeof(int32_t) * cnt, hipMemcpyDeviceToDevice, s));
    if (root_pivots_out) HIP_TRY(hipMemcpyAsync(root_pivots_out, b->q.pivots.p, sizeof(int64_t) * cnt, hipMemcpyDeviceToDevice, s));
    if (walk) {
        if (nodes_out) HIP_TRY(hipMemcpyAsync(nodes_out, t.d_used.p, sizeof(int64_t) * cnt, hipMemcpyDeviceToDevice, s));
        if (node_pivots_out) HIP_TRY(hipMemcpyAsync(node_pivots_out, t.q.pivots.p, sizeof(int64_t) * cnt, hipMemcpyDeviceToDevice, s));
    } else {
        if (nodes_out) HIP_TRY(hipMemsetAsync(nodes_out, 0, sizeof(int64_t) * cnt, s));
        if (node_pivots_out) HIP_TRY(hipMemsetAsync(node_pivots_out, 0, sizeof(int64_t) * cnt, s));
    }
    MilpSolutionArgs a{};
    a.n = n, a.h0 = h, a.hmax = hmax, a.overflow = YALPS_MILPDENSE_OVERFLOW;
    a.sign = D.sign, a.precision = precision;
    a.status = last.status.as<const int32_t>();
    a.result = last.result.as<const double>();
    a.best_h = walk ? t.d_best_h.as<const int32_t>() : nullptr;
    a.root_col0 = b->q.col0.as<const double>(), a.root_pos = b->q.pos.as<const int32_t>(), a.root_var = b->q.var.as<const int32_t>();
    a.tree_col0 = walk ? t.q.col0.as<const double>() : nullptr;
    a.tree_pos = walk ? t.q.pos.as<const int32_t>() : nullptr, a.tree_var = walk ? t.q.var.as<const int32_t>() : nullptr;
    a.x = n ? x_out : nullptr, a.objective = objective_out;
    a.status_out = status_out, a.nodes_out = reinterpret_cast<long long *>(nodes_out);
    a.node_pivots_out = reinterpret_cast<long long *>(node_pivots_out);
    HIP_TRY(hipEventRecord(b->ev0, s));
    if (lists) a.c = D.c, a.lb = D.lb, a.kind = D.kind;
    if (split) a.n_free = n_free, a.twin = D.twin;
    void (*const solution)(MilpSolutionArgs) = split ? free_kernels().solution : bounds ? bounds_kernels().solution : milp_dense_solution_kernel<SOLUTION_LANES>;
    solution<<<dim3((unsigned)count), dim3(SOLUTION_LANES), 0, s>>>(a);
    HIP_TRY(hipGetLastError());
    HIP_TRY(hipEventRecord(b->ev1, s));
    HIP_TRY(hipStreamSynchronize(s));
    HIP_TRY(hipEventElapsedTime(&tm.epilogue, b->ev0, b->ev1));
    char line[192];
    std::snprintf(line, sizeof line, "launch=%lld pass=0 kernel=milp_dense_%ssolution_kernel<%d> class=-1 trees=%d grid=%d lds=0 hist_cap=0\n",
                  (long long)t.launches++, split ? "free_" : bounds ? "bounds_" : "", SOLUTION_LANES, count, count);
    tm.epilogue_line = line;
    b->walked = walk;
    b->count = count;
    return 0;
}

void info_close(yalps_milpdense *b, const Times &tm) {
    const TreePass &t = b->t;
    char head[256];
    std::snprintf(head, sizeof head, "launches=%lld reruns=%zu overflows=%lld gpu_us=%lld root_us=%lld tree_us=%lld epilogue_us=%lld rerun_lps=[",
                  (long long)std::max<int64_t>(t.launches, tm.launches), t.rerun_ids.size() + tm.rerun_lps.size(), (long long)t.overflows,
                  (long long)std::llround((tm.root + t.gpu_ms + tm.epilogue) * 1000.0), (long long)std::llround(tm.root * 1000.0),
                  (long long)std::llround(t.gpu_ms * 1000.0), (long long)std::llround(tm.epilogue * 1000.0));
    b->info = head + join_ids(tm.rerun_lps) + "] rerun_trees=[" + join_ids(t.rerun_ids) + "]\n" + tm.root_lines + t.lines + tm.epilogue_line;
}

void call_stats(const yalps_milpdense *d, const Times &tm, int64_t *out) {
    if (!out) return;
    out[0] = (int64_t)(d->t.rerun_ids.size() + tm.rerun_lps.size());
    out[1] = std::max<int64_t>(d->t.launches, tm.launches);
    out[2] = d->t.overflows;
    out[3] = (int64_t)std::llround(tm.root * 1000.0);
    out[4] = (int64_t)std::llround(d->t.gpu_ms * 1000.0);
    out[5] = (int64_t)std::llround(tm.epilogue * 1000.0);
}

void destroy_impl(yalps_milpdense *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    release(b->q);
    release(b->t);
    release({&b->call, &b->rdesc});
    close_device(*b);
    delete b;
}
} // namespace

extern "C" {

const char *yalps_milpdense_last_error(void) { return g_err.c_str(); }

int32_t yalps_milpdense_validate(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c,
                                 const yalps_milpdense_operand *A_ub, const yalps_milpdense_operand *b_ub,
                                 const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq, int32_t n_integers,
                                 const int32_t *integers, int32_t n_binaries, const int32_t *binaries) {
    return validate(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, n_integers, integers, n_binaries, binaries);
}

int32_t yalps_milpdense_validate_bounds(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c,
                                        const yalps_milpdense_operand *A_ub, const yalps_milpdense_operand *b_ub,
                                        const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq,
                                        const yalps_milpdense_operand *lb, const yalps_milpdense_operand *ub, int32_t n_upper,
                                        const int32_t *upper_idx, int32_t n_integers, const int32_t *integers, int32_t n_binaries,
                                        const int32_t *binaries) {
    return validate_bounds(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, lb, ub, n_upper, upper_idx, n_integers, integers, n_binaries,
                           binaries);
}

int32_t yalps_milpdense_validate_free(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_milpdense_operand *c,
                                      const yalps_milpdense_operand *A_ub, const yalps_milpdense_operand *b_ub,
                                      const yalps_milpdense_operand *A_eq, const yalps_milpdense_operand *b_eq,
                                      const yalps_milpdense_operand *lb, const yalps_milpdense_operand *ub, int32_t n_upper,
                                      const int32_t *upper_idx, int32_t n_free, const int32_t *free_idx, int32_t n_integers,
                                      const int32_t *integers, int32_t n_binaries, const int32_t *binaries) {
    return validate_free(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, lb, ub, n_upper, upper_idx, n_free, free_idx, n_integers, integers,
                         n_binaries, binaries);
}

int32_t yalps_milpdense_create(int32_t device, void *hip_stream, yalps_milpdense **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_milpdense_create: out is NULL");
    *out = nullptr;
    const int rc = create_impl(device, hip_stream, out);
    if (rc && *out) { // a half-made handle is taken down again and the reason kept
        const std::string why = g_err;
        destroy_impl(*out);
        *out = nullptr;
        g_err = why;
    }
    return rc;
}

void yalps_milpdense_destroy(yalps_milpdense *d) { destroy_impl(d); }

int32_t yalps_milpdense_solve(yalps_milpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                              const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                              const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq,
                              const yalps_milpdense_operand *b_eq, int32_t n_integers, const int32_t *integers,
                              int32_t n_binaries, const int32_t *binaries, int32_t maximize, double precision,
                              double maxPivots, int32_t checkCycles, double tolerance, double maxIterations,
                              int32_t trace_cap, double *x_out, double *objective_out, int32_t *status_out,
                              int64_t *nodes_out, int64_t *node_pivots_out, int64_t *root_pivots_out,
                              int64_t *call_stats_out) {
    if (!d) return fail(YALPS_E_ARG, "yalps_milpdense_solve: handle is NULL");
    Times tm;
    const int32_t rc = solve_impl(d, "yalps_milpdense_solve", count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, n_integers, integers, n_binaries, binaries, maximize,
                                  precision, maxPivots, checkCycles, tolerance, maxIterations, trace_cap, x_out, objective_out,
                                  status_out, nodes_out, node_pivots_out, root_pivots_out, tm);
    if (rc) d->count = 0; // (no last solve to read from)
    info_close(d, tm);
    call_stats(d, tm, call_stats_out);
    return rc;
}

int32_t yalps_milpdense_solve_bounds(yalps_milpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                     const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                                     const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq,
                                     const yalps_milpdense_operand *b_eq, const yalps_milpdense_operand *lb,
                                     const yalps_milpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx,
                                     int32_t n_integers, const int32_t *integers, int32_t n_binaries, const int32_t *binaries,
                                     int32_t maximize, double precision, double maxPivots, int32_t checkCycles, double tolerance,
                                     double maxIterations, int32_t trace_cap, double *x_out, double *objective_out,
                                     int32_t *status_out, int64_t *nodes_out, int64_t *node_pivots_out, int64_t *root_pivots_out,
                                     int64_t *call_stats_out) {
    if (!d) return fail(YALPS_E_ARG, "yalps_milpdense_solve_bounds: handle is NULL");
    Times tm;
    const int32_t rc = solve_impl(d, "yalps_milpdense_solve_bounds", count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, n_integers, integers,
                                  n_binaries, binaries, maximize, precision, maxPivots, checkCycles, tolerance, maxIterations, trace_cap,
                                  x_out, objective_out, status_out, nodes_out, node_pivots_out, root_pivots_out, tm, lb, ub, n_upper,
                                  upper_idx);
    if (rc) d->count = 0; // (no last solve to read from)
    info_close(d, tm);
    call_stats(d, tm, call_stats_out);
    return rc;
}

int32_t yalps_milpdense_solve_free(yalps_milpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                   const yalps_milpdense_operand *c, const yalps_milpdense_operand *A_ub,
                                   const yalps_milpdense_operand *b_ub, const yalps_milpdense_operand *A_eq,
                                   const yalps_milpdense_operand *b_eq, const yalps_milpdense_operand *lb,
                                   const yalps_milpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx, int32_t n_free,
                                   const int32_t *free_idx, int32_t n_integers, const int32_t *integers, int32_t n_binaries,
                                   const int32_t *binaries, int32_t maximize, double precision, double maxPivots, int32_t checkCycles,
                                   double tolerance, double maxIterations, int32_t trace_cap, double *x_out, double *objective_out,
                                   int32_t *status_out, int64_t *nodes_out, int64_t *node_pivots_out, int64_t *root_pivots_out,
                                   int64_t *call_stats_out) {
    if (!d) return fail(YALPS_E_ARG, "yalps_milpdense_solve_free: handle is NULL");
    Times tm;
    const int32_t rc = solve_impl(d, "yalps_milpdense_solve_free", count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, n_integers, integers,
                                  n_binaries, binaries, maximize, precision, maxPivots, checkCycles, tolerance, maxIterations, trace_cap,
                                  x_out, objective_out, status_out, nodes_out, node_pivots_out, root_pivots_out, tm, lb, ub, n_upper,
                                  upper_idx, n_free, free_idx);
    if (rc) d->count = 0; // (no last solve to read from)
    info_close(d, tm);
    call_stats(d, tm, call_stats_out);
    return rc;
}

int32_t yalps_milpdense_overflowed(const yalps_milpdense *d, int32_t *ids, int32_t cap) {
    if (!d) return fail(YALPS_E_ARG, "yalps_milpdense_overflowed: handle is NULL");
    if (d->count == 0) return 0;
    for (size_t k = 0; ids && k < d->overflowed.size() && k < (size_t)std::max(0, cap); k++) ids[k] = d->overflowed[k];
    return (int32_t)d->overflowed.size();
}

int32_t yalps_milpdense_solution(yalps_milpdense *d, int32_t i, int32_t *status_out, double *result_out, int32_t *height_out,
                                 double *col0, int32_t *positionOfVariable, int32_t *variableAtPosition) {
    if (!d || i < 0 || i >= d->count) return fail(YALPS_E_ARG, "yalps_milpdense_solution: no such MILP in the last solve");
    hipStream_t s = d->stream;
    HIP_TRY(hipSetDevice(d->device));
    const QueueBufs &last = d->walked ? d->t.q : d->q;
    int32_t st = 0, bh = 0;
    double res = NAN;
    HIP_TRY(hipMemcpyAsync(&st, last.status.as<const int32_t>() + i, sizeof st, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipMemcpyAsync(&res, last.result.as<const double>() + i, sizeof res, hipMemcpyDeviceToHost, s));
    if (d->walked) HIP_TRY(hipMemcpyAsync(&bh, d->t.d_best_h.as<const int32_t>() + i, sizeof bh, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    if (st < 0 || st > YALPS_MILPDENSE_TIMEDOUT) st = YALPS_MILPDENSE_OVERFLOW, res = NAN, bh = 0; // (the host gave this tree up)
    const bool root = bh <= 0; // no incumbent: bestTableau is the root's (src/branchAndCut.ts:119)
    const size_t hs = root ? (size_t)d->h0 : (size_t)d->h0 + 2 * (size_t)d->nints; // the slices' stride follows the buffer
    const size_t h = root ? (size_t)d->h0 : (size_t)bh, np = (size_t)d->w + h;
    const QueueBufs &from = root ? d->q : d->t.q;
    if (status_out) *status_out = st;
    if (result_out) *result_out = res;
    if (height_out) *height_out = (int32_t)h;
    if (col0)
        HIP_TRY(hipMemcpyAsync(col0, from.col0.as<const double>() + (size_t)i * ((hs + 1) & ~(size_t)1), sizeof(double) * h, hipMemcpyDeviceToHost, s));
    if (positionOfVariable)
        HIP_TRY(hipMemcpyAsync(positionOfVariable, from.pos.as<const int32_t>() + (size_t)i * ((size_t)d->w + hs), sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    if (variableAtPosition)
        HIP_TRY(hipMemcpyAsync(variableAtPosition, from.var.as<const int32_t>() + (size_t)i * ((size_t)d->w + hs), sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int32_t yalps_milpdense_trace(yalps_milpdense *d, int32_t i, int32_t *count_out, double *eval, int32_t *status, double *result,
                              int64_t *pivots, int32_t *height, int32_t *cut_sign, int32_t *cut_var, double *cut_val) {
    if (!d || i < 0 || i >= d->count) return fail(YALPS_E_ARG, "yalps_milpdense_trace: no such MILP in the last solve");
    int32_t cnt = 0;
    std::vector<double> slice;
    int32_t maxcuts = 1;
    if (d->walked && d->t.trace_cap > 0 && d->t.q.h_status[(size_t)i] != TREE_OVERFLOW) {
        const TreeDesc &t = d->t.trees[(size_t)i];
        maxcuts = t.maxcuts;
        long long used = 0;
        hipStream_t s = d->stream;
        HIP_TRY(hipSetDevice(d->device));
        HIP_TRY(hipMemcpyAsync(&used, d->t.d_used.as<const long long>() + i, sizeof used, hipMemcpyDeviceToHost, s));
        HIP_TRY(hipStreamSynchronize(s));
        cnt = (int32_t)std::max<long long>(0, std::min<long long>(used, d->t.trace_cap));
        slice.resize((size_t)cnt * (4 + 2 * (size_t)maxcuts));
        if (cnt) {
            HIP_TRY(hipMemcpyAsync(slice.data(), d->t.d_trace.as<const double>() + t.trace_off, sizeof(double) * slice.size(), hipMemcpyDeviceToHost, s));
            HIP_TRY(hipStreamSynchronize(s));
        }
    }
    if (count_out) *count_out = cnt;
    tree_trace_out(slice.data(), maxcuts, cnt, d->h0, eval, status, result, pivots, height, cut_sign, cut_var, cut_val);
    return 0;
}

int32_t yalps_milpdense_info(const yalps_milpdense *d, char *buf, int32_t len) {
    if (!d || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_milpdense_info: bad argument");
    return info_out(d->info, buf, len);
}

} // extern "C"
