// lp_dense.hip -- libyalps_lpdense.so: a batch of dense LPs of one shape, from device operands to device answers (include/yalps_lpdense.h)
// C ABI, host side and the lp_dense_kernel instantiations.  A library of its own: nothing here is linked into the others, and
// the pivot loop is libyalps_hip.so's wg_simplex.cuh, included unchanged.  Size classes, the pass and the rerun protocol are
// wg_queue_host.inc with this library's kernel table; one shape per call means one class and at most one launch per pass.
// Nothing of an LP crosses PCIe but its status: the operands are read where they lie, x / objective are written by the
// kernel, status / pivots are copied device to device, and column 0 and the permutations stay on the device until
// yalps_lpdense_solution asks for them.
// A call with bounds (lb / ub) runs lp_dense_bounds_kernel, whose six forms are libyalps_lpdense_bounds.so's: this library links
// it and takes the kernels' pointers from yalps_lpdense_bounds_forms, so its own code object holds the boundless forms alone.
// A call with free variables (n_free > 0) runs lp_dense_free_kernel, libyalps_lpdense_free.so's six forms, taken the same way.
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

#include "../../include/yalps_lpdense.h"

#pragma clang fp contract(off)

namespace {
#include "common.cuh"

#include "wg_simplex.cuh"
#include "lp_dense_kernel.cuh"
#include "wg_queue_host.inc"
#include "dense_host.inc"

static_assert(YALPS_LPDENSE_MAX_BYTES == QUEUE_MAX_BYTES, "include/yalps_lpdense.h");
const KernelTable<DenseLaunch> kDenseKernels = QUEUE_KERNEL_TABLE(lp_dense_kernel);
struct X { // (dense_host.inc)
    static constexpr const char *name = "yalps_lpdense";
    using Operand = yalps_lpdense_operand;
};
} // namespace

extern "C" void yalps_lpdense_bounds_forms(void *out[6]); // lp_dense_bounds.hip
extern "C" void yalps_lpdense_free_forms(void *out[6]);   // lp_dense_free.hip

namespace {
// the same table over libyalps_lpdense_bounds.so's kernels
const KernelTable<DenseLaunch> &bounds_kernels() {
    static const KernelTable<DenseLaunch> table = adopt_forms(kDenseKernels, "lp_dense_bounds_kernel", yalps_lpdense_bounds_forms);
    return table;
}
// and over libyalps_lpdense_free.so's
const KernelTable<DenseLaunch> &free_kernels() {
    static const KernelTable<DenseLaunch> table = adopt_forms(kDenseKernels, "lp_dense_free_kernel", yalps_lpdense_free_forms);
    return table;
}
} // namespace

struct yalps_lpdense : QueueDevice {
    QueueBufs q;
    DevBuf call;
    DenseCall desc;               // the call's description as it was uploaded
    std::vector<int32_t> upper_idx; // the call's index lists (bound rows, free variables, the twin of every variable), kept until their upload has gone
    // the last solve
    int32_t w = 0, h = 0, count = 0;
    std::string info;
};

namespace {
int validate(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
             const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq, int32_t n_upper = 0,
             int32_t n_free = 0) {
    if (count < 0) return fail(YALPS_E_ARG, "yalps_lpdense: count < 0");
    if (n < 0 || m_ub < 0 || m_eq < 0) return fail(YALPS_E_ARG, "yalps_lpdense: n, m_ub and m_eq must be at least 0");
    if (n_upper < 0) return fail(YALPS_E_ARG, "yalps_lpdense: n_upper < 0");
    if (n_free < 0) return fail(YALPS_E_ARG, "yalps_lpdense: n_free < 0");
    const int64_t w = (int64_t)n + 1 + (int64_t)n_free, h = 1 + (int64_t)m_ub + 2 * (int64_t)m_eq + (int64_t)n_upper;
    if (w > INT32_MAX || h > INT32_MAX || 8 * w * h > YALPS_LPDENSE_MAX_BYTES)
        return fail(YALPS_E_ARG, "yalps_lpdense: tableau of " + std::to_string(h) + " x " + std::to_string(w) + " doubles is above the limit of " +
                                     std::to_string((long long)YALPS_LPDENSE_MAX_BYTES) + " bytes");
    return check_operands<X>(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq);
}

// the bounds of a call: lb / ub may be NULL descriptors (absent); upper_idx is host memory, ascending, inside 0 .. n-1
int validate_bounds(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                    const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq,
                    const yalps_lpdense_operand *lb, const yalps_lpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx,
                    int32_t n_free = 0, const int32_t *free_idx = nullptr) {
    if (int rc = validate(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, n_upper, n_free)) return rc;
    const auto nothing = [](int32_t) { return 0; };
    if (int rc = check_bounds<X>(count, n, lb, ub, n_upper, upper_idx, nothing)) return rc;
    // the free variables: host memory, ascending, inside 0 .. n-1 (the width that counts their twins is checked above)
    return check_index_list<X>("free_idx", n_free, free_idx, n, nothing);
}

int create_impl(int32_t device, void *hip_stream, yalps_lpdense **out) {
    yalps_lpdense *b = new yalps_lpdense();
    *out = b;
    // (test hooks: a grid smaller than the card, one per_cu for every class, so that a workgroup takes several LPs of any class;
    // read and refused in front of the device, 0 or unset: the card's own table)
    const int per_cu = env_int("YALPS_LPDENSE_PER_CU", 0), cus = env_int("YALPS_LPDENSE_CUS", 0);
    if (per_cu < 0 || per_cu > 8) return fail(YALPS_E_ARG, "YALPS_LPDENSE_PER_CU: " + std::to_string(per_cu) + " is outside 0..8 (0: unset)");
    if (cus < 0) return fail(YALPS_E_ARG, "YALPS_LPDENSE_CUS: " + std::to_string(cus) + " is negative");
    if (int rc = open_device(*b, device, hip_stream)) return rc;
    if (hip_stream == static_cast<void *>(hipStreamLegacy)) b->stream = nullptr; // the device's default stream, by its own name
    b->q.hist_first = std::max(1, env_int("YALPS_LPDENSE_HIST", (int)HIST_FIRST)); // (test hook: forces the rerun)
    if (cus) b->num_cus = std::min(cus, b->num_cus);
    if (per_cu)
        for (int k = 0; k < NCLASS; k++) b->per_cu[k] = std::min(per_cu, kClasses[k].per_cu);
    if (int rc = raise_lds_limit(kDenseKernels)) return rc;
    if (int rc = raise_lds_limit(bounds_kernels())) return rc;
    return raise_lds_limit(free_kernels());
}

int solve_impl(yalps_lpdense *b, const char *entry, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c,
               const yalps_lpdense_operand *A_ub, const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
               const yalps_lpdense_operand *b_eq, int32_t maximize, double precision, double maxPivots, int32_t checkCycles, int32_t keep,
               double *x_out, double *objective_out, int32_t *status_out, int64_t *pivots_out, double *ineqlin_out,
               double *eqlin_out, double *reduced_out, float *gpu_ms_out, const yalps_lpdense_operand *lb = nullptr,
               const yalps_lpdense_operand *ub = nullptr, int32_t n_upper = 0, const int32_t *upper_idx = nullptr,
               double *upper_out = nullptr, int32_t n_free = 0, const int32_t *free_idx = nullptr) {
    if (int rc = validate_bounds(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, lb, ub, n_upper, upper_idx, n_free, free_idx)) return rc;
    // (a free variable: lp_dense_free_kernel; else either descriptor: lp_dense_bounds_kernel; neither: the kernels and the bits of before)
    const bool bounds = lb || ub;
    b->count = 0;
    b->q.keep = keep != 0;
    b->info = "launches=0 reruns=0\n";
    if (gpu_ms_out) *gpu_ms_out = 0.f;
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
                    {"x_out", n ? x_out : nullptr},
                    {"objective_out", objective_out},
                    {"status_out", status_out},
                    {"pivots_out", pivots_out},
                    {"ineqlin_out", m_ub ? ineqlin_out : nullptr},
                    {"eqlin_out", m_eq ? eqlin_out : nullptr},
                    {"reduced_out", n ? reduced_out : nullptr},
                    {"lb", lb && n ? lb->ptr : nullptr},
                    {"ub", ub && n_upper ? ub->ptr : nullptr},
                    {"upper_out", n_upper ? upper_out : nullptr}};
    for (const auto &a : pointers)
        if (int rc = check_pointer(b->device, entry, a.name, a.p)) return rc;

    hipStream_t s = b->stream;
    const int32_t w = n + 1 + n_free, h = 1 + m_ub + 2 * m_eq + n_upper;
    const size_t cnt = (size_t)count, heven = ((size_t)h + 1) & ~(size_t)1, perm = (size_t)w + (size_t)h;
    const int cls = lp_class(w, h);
    const bool aux = cls == HBM_CLASS && lp_aux_hbm(w, h);
    // x / objective of a call that does not want them: rows of the handle's own, behind the call's description
    const size_t call_bytes = (sizeof(DenseCall) + 15) & ~(size_t)15;
    const size_t own_x = x_out || !n ? 0 : sizeof(double) * cnt * (size_t)n, own_obj = objective_out ? 0 : sizeof(double) * cnt;
    const size_t own_end = (own_x + own_obj + 15) & ~(size_t)15, idx_bytes = sizeof(int32_t) * ((size_t)n_upper + (n_free ? (size_t)n_free + (size_t)n : 0)); // (the index lists last)
    if (int rc = ensure(b->call, call_bytes + own_end + idx_bytes)) return rc;
    if (int rc = ensure_outputs(b->q, cnt, heven * cnt, perm * cnt, (size_t)w * (size_t)h * cnt)) return rc;
    char *behind = b->call.as<char>() + call_bytes;
    DenseCall &D = b->desc;
    D = DenseCall{};
    D.n = n;
    D.m_ub = m_ub;
    D.m_eq = m_eq;
    D.aux_hbm = aux ? 1 : 0;
    D.sign = maximize ? 1.0 : -1.0;
    D.precision = precision;
    D.max_pivots = maxPivots;
    D.c = operand(c, true);
    D.A_ub = operand(A_ub, false);
    D.b_ub = operand(b_ub, true);
    D.A_eq = operand(A_eq, false);
    D.b_eq = operand(b_eq, true);
    D.x = x_out ? x_out : reinterpret_cast<double *>(behind);
    D.objective = objective_out ? objective_out : reinterpret_cast<double *>(behind + own_x);
    D.ineqlin = m_ub ? ineqlin_out : nullptr; // (an output without an element is not written, whatever was passed)
    D.eqlin = m_eq ? eqlin_out : nullptr;
    D.reduced = n ? reduced_out : nullptr;
    if (lb && n) D.lb = operand(lb, true);
    if (ub && n_upper) D.ub = operand(ub, true);
    D.n_upper = n_upper;
    D.upper = n_upper ? upper_out : nullptr;
    D.n_free = n_free;
    if (idx_bytes) { // upper_idx[n_upper], then free_idx[n_free] and twin[n] where the call has free variables: one upload
        b->upper_idx.assign(upper_idx, upper_idx + n_upper);
        const int32_t *lists = reinterpret_cast<const int32_t *>(behind + own_end);
        if (n_upper) D.upper_idx = lists;
        if (n_free) {
            b->upper_idx.insert(b->upper_idx.end(), free_idx, free_idx + n_free);
            b->upper_idx.resize((size_t)n_upper + (size_t)n_free + (size_t)n, -1);
            for (int32_t t = 0; t < n_free; t++) b->upper_idx[(size_t)n_upper + (size_t)n_free + (size_t)free_idx[t]] = 1 + n + t;
            D.free_idx = lists + n_upper;
            D.twin = lists + n_upper + n_free;
        }
        HIP_TRY(hipMemcpyAsync(behind + own_end, b->upper_idx.data(), idx_bytes, hipMemcpyHostToDevice, s));
    }
    HIP_TRY(hipMemcpyAsync(b->call.p, &D, sizeof D, hipMemcpyHostToDevice, s));
    if (int rc = reset_status(b->q, s, cnt)) return rc;
    b->w = w;
    b->h = h;
    b->count = count;

    // an LP whose phase outran the history runs again from the operands, which nothing has touched
    std::string text;
    QueueRun run;
    const int rc = run_queue(
        *b, b->q, n_free ? free_kernels() : bounds ? bounds_kernels() : kDenseKernels, QueueText{"yalps_lpdense", true, "yalps_lpdense_solve", "LP"}, cnt,
        [&](int32_t, int *iw, int *ih) { return *iw = w, *ih = h, checkCycles != 0; },
        [&](DenseLaunch &a) { a.call = b->call.as<const DenseCall>(); },
        [&] { // on the way back with the statuses, device to device (a pass that reruns some leaves them to the next one)
            if (status_out) HIP_TRY(hipMemcpyAsync(status_out, b->q.status.p, sizeof(int32_t) * cnt, hipMemcpyDeviceToDevice, s));
            if (pivots_out) HIP_TRY(hipMemcpyAsync(pivots_out, b->q.pivots.p, sizeof(int64_t) * cnt, hipMemcpyDeviceToDevice, s));
            return 0;
        },
        [&](const Launch &L, const std::string &kernel, int pass, int launch, long long hist_cap) {
            char line[256];
            std::snprintf(line, sizeof line, "launch=%d pass=%d kernel=%s class=%d aux=%d lps=%zu grid=%d lds=%zu hist_cap=%lld\n", launch,
                          pass, kernel.c_str(), L.cls, aux ? 1 : 0, L.items.size(), L.grid, L.shmem, hist_cap);
            text += line;
        },
        run);
    if (rc) return rc;
    b->info = "launches=" + std::to_string(run.launches) + " reruns=" + std::to_string(run.reruns.size()) + " rerun_lps=[" +
              join_ids(run.reruns) + "]\n" + text;
    if (gpu_ms_out) *gpu_ms_out = run.ms;
    return 0;
}

void destroy_impl(yalps_lpdense *b) {
    if (!b) return;
    (void)hipSetDevice(b->device);
    if (b->stream) (void)hipStreamSynchronize(b->stream);
    release(b->q);
    release({&b->call});
    close_device(*b);
    delete b;
}
} // namespace

extern "C" {

const char *yalps_lpdense_last_error(void) { return g_err.c_str(); }

int32_t yalps_lpdense_validate(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c,
                               const yalps_lpdense_operand *A_ub, const yalps_lpdense_operand *b_ub,
                               const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq) {
    return validate(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq);
}

int32_t yalps_lpdense_validate_bounds(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c,
                                      const yalps_lpdense_operand *A_ub, const yalps_lpdense_operand *b_ub,
                                      const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq,
                                      const yalps_lpdense_operand *lb, const yalps_lpdense_operand *ub, int32_t n_upper,
                                      const int32_t *upper_idx) {
    return validate_bounds(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, lb, ub, n_upper, upper_idx);
}

int32_t yalps_lpdense_validate_free(int32_t count, int32_t n, int32_t m_ub, int32_t m_eq, const yalps_lpdense_operand *c,
                                    const yalps_lpdense_operand *A_ub, const yalps_lpdense_operand *b_ub,
                                    const yalps_lpdense_operand *A_eq, const yalps_lpdense_operand *b_eq,
                                    const yalps_lpdense_operand *lb, const yalps_lpdense_operand *ub, int32_t n_upper,
                                    const int32_t *upper_idx, int32_t n_free, const int32_t *free_idx) {
    return validate_bounds(count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, lb, ub, n_upper, upper_idx, n_free, free_idx);
}

int32_t yalps_lpdense_create(int32_t device, void *hip_stream, yalps_lpdense **out) {
    if (!out) return fail(YALPS_E_ARG, "yalps_lpdense_create: out is NULL");
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

void yalps_lpdense_destroy(yalps_lpdense *d) { destroy_impl(d); }

int32_t yalps_lpdense_solve(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                            const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                            const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                            const yalps_lpdense_operand *b_eq, int32_t maximize, double precision, double maxPivots,
                            int32_t checkCycles, int32_t keep_tableaux, double *x_out, double *objective_out,
                            int32_t *status_out, int64_t *pivots_out, float *gpu_ms_out) {
    if (!d) return fail(YALPS_E_ARG, "yalps_lpdense_solve: handle is NULL");
    const int32_t rc = solve_impl(d, "yalps_lpdense_solve", count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, maximize, precision, maxPivots,
                                  checkCycles, keep_tableaux, x_out, objective_out, status_out, pivots_out, nullptr, nullptr, nullptr,
                                  gpu_ms_out);
    if (rc) d->count = 0; // (no last solve to read from)
    return rc;
}

int32_t yalps_lpdense_solve_duals(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                  const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                                  const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                                  const yalps_lpdense_operand *b_eq, int32_t maximize, double precision, double maxPivots,
                                  int32_t checkCycles, int32_t keep_tableaux, double *x_out, double *objective_out,
                                  int32_t *status_out, int64_t *pivots_out, double *ineqlin_out, double *eqlin_out,
                                  double *reduced_out, float *gpu_ms_out) {
    if (!d) return fail(YALPS_E_ARG, "yalps_lpdense_solve_duals: handle is NULL");
    const int32_t rc = solve_impl(d, "yalps_lpdense_solve_duals", count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, maximize, precision,
                                  maxPivots, checkCycles, keep_tableaux, x_out, objective_out, status_out, pivots_out, ineqlin_out,
                                  eqlin_out, reduced_out, gpu_ms_out);
    if (rc) d->count = 0; // (no last solve to read from)
    return rc;
}

int32_t yalps_lpdense_solve_bounds(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                   const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                                   const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                                   const yalps_lpdense_operand *b_eq, const yalps_lpdense_operand *lb,
                                   const yalps_lpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx, int32_t maximize,
                                   double precision, double maxPivots, int32_t checkCycles, int32_t keep_tableaux, double *x_out,
                                   double *objective_out, int32_t *status_out, int64_t *pivots_out, double *ineqlin_out,
                                   double *eqlin_out, double *reduced_out, double *upper_out, float *gpu_ms_out) {
    if (!d) return fail(YALPS_E_ARG, "yalps_lpdense_solve_bounds: handle is NULL");
    const int32_t rc = solve_impl(d, "yalps_lpdense_solve_bounds", count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, maximize, precision,
                                  maxPivots, checkCycles, keep_tableaux, x_out, objective_out, status_out, pivots_out, ineqlin_out,
                                  eqlin_out, reduced_out, gpu_ms_out, lb, ub, n_upper, upper_idx, upper_out);
    if (rc) d->count = 0; // (no last solve to read from)
    return rc;
}

int32_t yalps_lpdense_solve_free(yalps_lpdense *d, int32_t count, int32_t n, int32_t m_ub, int32_t m_eq,
                                 const yalps_lpdense_operand *c, const yalps_lpdense_operand *A_ub,
                                 const yalps_lpdense_operand *b_ub, const yalps_lpdense_operand *A_eq,
                                 const yalps_lpdense_operand *b_eq, const yalps_lpdense_operand *lb,
                                 const yalps_lpdense_operand *ub, int32_t n_upper, const int32_t *upper_idx, int32_t n_free,
                                 const int32_t *free_idx, int32_t maximize, double precision, double maxPivots, int32_t checkCycles,
                                 int32_t keep_tableaux, double *x_out, double *objective_out, int32_t *status_out, int64_t *pivots_out,
                                 double *ineqlin_out, double *eqlin_out, double *reduced_out, double *upper_out, float *gpu_ms_out) {
    if (!d) return fail(YALPS_E_ARG, "yalps_lpdense_solve_free: handle is NULL");
    const int32_t rc = solve_impl(d, "yalps_lpdense_solve_free", count, n, m_ub, m_eq, c, A_ub, b_ub, A_eq, b_eq, maximize, precision,
                                  maxPivots, checkCycles, keep_tableaux, x_out, objective_out, status_out, pivots_out, ineqlin_out,
                                  eqlin_out, reduced_out, gpu_ms_out, lb, ub, n_upper, upper_idx, upper_out, n_free, free_idx);
    if (rc) d->count = 0; // (no last solve to read from)
    return rc;
}

int32_t yalps_lpdense_solution(yalps_lpdense *d, int32_t i, double *col0, int32_t *positionOfVariable, int32_t *variableAtPosition) {
    if (!d || i < 0 || i >= d->count) return fail(YALPS_E_ARG, "yalps_lpdense_solution: no such LP in the last solve");
    const size_t h = (size_t)d->h, heven = (h + 1) & ~(size_t)1, np = (size_t)d->w + h;
    hipStream_t s = d->stream;
    HIP_TRY(hipSetDevice(d->device));
    if (col0) HIP_TRY(hipMemcpyAsync(col0, d->q.col0.as<const double>() + (size_t)i * heven, sizeof(double) * h, hipMemcpyDeviceToHost, s));
    if (positionOfVariable)
        HIP_TRY(hipMemcpyAsync(positionOfVariable, d->q.pos.as<const int32_t>() + (size_t)i * np, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    if (variableAtPosition)
        HIP_TRY(hipMemcpyAsync(variableAtPosition, d->q.var.as<const int32_t>() + (size_t)i * np, sizeof(int32_t) * np, hipMemcpyDeviceToHost, s));
    HIP_TRY(hipStreamSynchronize(s));
    return 0;
}

int32_t yalps_lpdense_tableau(yalps_lpdense *d, int32_t i, double *matrix) {
    if (!d || i < 0 || i >= d->count || !matrix) return fail(YALPS_E_ARG, "yalps_lpdense_tableau: no such LP in the last solve");
    if (!d->q.keep) return fail(YALPS_E_ARG, "yalps_lpdense_tableau: the last solve did not keep its tableaux (keep_tableaux)");
    const size_t wh = (size_t)d->w * (size_t)d->h;
    HIP_TRY(hipSetDevice(d->device));
    HIP_TRY(hipMemcpyAsync(matrix, d->q.tab.as<const double>() + (size_t)i * wh, sizeof(double) * wh, hipMemcpyDeviceToHost, d->stream));
    HIP_TRY(hipStreamSynchronize(d->stream));
    return 0;
}

int32_t yalps_lpdense_info(const yalps_lpdense *d, char *buf, int32_t len) {
    if (!d || !buf || len < 1) return fail(YALPS_E_ARG, "yalps_lpdense_info: bad argument");
    return info_out(d->info, buf, len);
}

} // extern "C"
